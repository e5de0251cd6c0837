"""CPU: the ctypes prototype table (neuraloc_amd._lib.PROTOTYPES) IS include/nocf.h -- every entry declared, with the header's argument count,
argument kinds (pointer / integer / double, with their byte sizes; the struct behind a Nocf* pointer) and return kind; every declaration in the
table or in UNBOUND; and the loaded library carries the table.  A ctypes prototype that disagrees with the header does not raise: it hands a
kernel a wrong row count or a wrong pointer."""
import ctypes as C
import os
import re

import pytest

import __graft_entry__ as entry
from neuraloc_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = ("NocfPhi64", "NocfProb64", "NocfPhi", "NocfProb")
# declared in nocf.h and called by no file under neuraloc_amd/ (tests and tools bind them where they use them)
UNBOUND = ("nocf_debug_noise_words", "nocf_debug_set_timeline_buffer")
C_SCALARS = {"int": ("int", 4), "int32_t": ("int", 4), "uint32_t": ("int", 4), "int64_t": ("int", 8), "uint64_t": ("int", 8),
             "size_t": ("int", C.sizeof(C.c_size_t)), "double": ("double", 8), "float": ("float", 4)}


def c_kind(text):
    """a C parameter or return type (the parameter's name may follow) -> (kind, bytes, struct or None); None for void"""
    text = re.sub(r"\[[^\]]*\]", "*", text)                           # (an array parameter, `int32_t out[12]`, is a pointer)
    words = re.sub(r"\b(const|struct|restrict)\b", " ", text).replace("*", " * ").split()
    if "*" in words:
        return ("pointer", C.sizeof(C.c_void_p), words[0] if words[0] in STRUCTS else None)
    if words[0] == "void":
        return None
    return C_SCALARS[words[0]] + (None,)


def ctypes_kind(t):
    if t is None:
        return None
    if t in (C.c_void_p, C.c_char_p):
        return ("pointer", C.sizeof(t), None)
    if hasattr(t, "contents"):                                         # a POINTER(...)
        target = t._type_
        return ("pointer", C.sizeof(t), target.__name__ if issubclass(target, C.Structure) else None)
    if t is C.c_double:
        return ("double", 8, None)
    if t is C.c_float:
        return ("float", 4, None)
    assert t._type_ in "bBhHiIlLqQ", t
    return ("int", C.sizeof(t), None)


def declarations():
    """name -> (return kind, [argument kinds]) of every function include/nocf.h declares, comments stripped"""
    hdr = open(os.path.join(REPO, "include", "nocf.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*", " ", hdr)
    hdr = re.sub(r"^\s*#[^\n]*", " ", hdr, flags=re.M)
    hdr = re.sub(r"typedef\s+struct\s+\w+\s*\{.*?\}\s*\w+\s*;", " ", hdr, flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"([\w\s\*]+?)\b(nocf_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", hdr):
        assert name not in out, name
        args = args.strip()
        out[name] = (c_kind(ret), [] if args in ("", "void") else [c_kind(a) for a in args.split(",")])
    return out


def mismatches(name, proto, decl):
    """what is wrong with the ctypes prototype (restype, argtypes) of `name` against its declaration; [] when nothing is"""
    restype, argtypes = proto
    ret, args = decl
    bad = []
    if ctypes_kind(restype) != ret:
        bad.append(f"{name}: returns {ret} in the header, {ctypes_kind(restype)} in the table")
    if len(argtypes) != len(args):
        return bad + [f"{name}: {len(args)} arguments in the header, {len(argtypes)} in the table"]
    for i, (t, want) in enumerate(zip(argtypes, args)):
        if ctypes_kind(t) != want:
            bad.append(f"{name}: argument {i} is {want} in the header, {ctypes_kind(t)} in the table")
    return bad


@pytest.fixture(scope="module")
def L():
    entry.build()
    return _lib.lib()


def test_the_header_parses():
    decl = declarations()
    assert len(decl) == 100
    assert decl["nocf_version"] == (("int", 4, None), [])
    assert decl["nocf_last_rollout_kernel"][0] == ("pointer", 8, None)
    assert decl["nocf_debug_reload_env"] == (None, [])
    assert decl["nocf_rollout_f64"][1][:4] == [("pointer", 8, "NocfPhi64"), ("pointer", 8, "NocfProb64"), ("pointer", 8, None), ("int", 8, None)]
    assert decl["nocf_rollout_noisy_f32"][1][3:7] == [("pointer", 8, None), ("int", 8, None), ("int", 8, None), ("int", 8, None)]
    assert decl["nocf_rollout_f32"][1][4:9] == [("double", 8, None), ("double", 8, None), ("int", 4, None), ("int", 4, None), ("pointer", 8, None)]


def test_every_prototype_is_the_declaration():
    decl = declarations()
    bad = []
    for name, proto in _lib.PROTOTYPES.items():
        if name not in decl:
            bad.append(f"{name}: in the table, not declared in nocf.h")
        else:
            bad += mismatches(name, proto, decl[name])
    assert not bad, "\n".join(bad)


def test_every_declaration_is_bound_or_listed():
    decl = declarations()
    assert not set(UNBOUND) & set(_lib.PROTOTYPES)
    assert set(UNBOUND) <= set(decl)
    assert set(decl) == set(_lib.PROTOTYPES) | set(UNBOUND), sorted(set(decl) ^ (set(_lib.PROTOTYPES) | set(UNBOUND)))
    # UNBOUND is what no file of the package mentions
    pkg = os.path.join(REPO, "neuraloc_amd")
    text = "".join(open(os.path.join(root, f)).read() for root, _, files in os.walk(pkg) for f in files if f.endswith(".py"))
    for name in UNBOUND:
        assert name not in text, name
    assert set(_lib._REQUIRED) <= set(_lib.PROTOTYPES)


def test_the_loaded_library_carries_the_table(L):
    for name, (restype, argtypes) in _lib.PROTOTYPES.items():
        assert hasattr(L, name), name                                  # (the shipped library exports all of them)
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == list(argtypes), name


def _narrowed(proto):
    restype, argtypes = proto
    i = argtypes.index(C.c_int64)
    return restype, argtypes[:i] + [C.c_int32] + argtypes[i + 1:]


def _dropped(proto):
    return proto[0], proto[1][:-1]


def _other_struct(proto):
    restype, argtypes = proto
    i = argtypes.index(C.POINTER(_lib.NocfPhi))
    return restype, argtypes[:i] + [C.POINTER(_lib.NocfPhi64)] + argtypes[i + 1:]


@pytest.mark.parametrize("mutate, told", [(_narrowed, "argument 4 is ('int', 8, None) in the header, ('int', 4, None) in the table"),
                                          (_dropped, "19 arguments in the header, 18 in the table"),
                                          (_other_struct, "argument 0 is ('pointer', 8, 'NocfPhi') in the header, ('pointer', 8, 'NocfPhi64')")],
                         ids=["int64-as-int32", "one-argument-dropped", "NocfPhi-as-NocfPhi64"])
def test_the_comparator_reports_a_wrong_prototype(mutate, told):
    name = "nocf_rollout_disturbed_f32"
    decl = declarations()[name]
    restype, argtypes = _lib.PROTOTYPES[name]
    assert mismatches(name, (restype, list(argtypes)), decl) == []
    bad = mismatches(name, mutate((restype, list(argtypes))), decl)
    assert len(bad) == 1 and told in bad[0], bad
    assert list(_lib.PROTOTYPES[name][1]) == list(argtypes)           # (the table itself was not touched)
