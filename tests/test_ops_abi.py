"""The C ABI of libkfops.so is written down twice: as prototypes in
kubeflow_amd/ops/csrc/kf_ops.h (which every kernel file compiles against)
and as ctypes argtypes in kubeflow_amd/ops/_backend.py. A disagreement is not
a test failure on its own: it is a wrong pointer handed to a kernel. This
test parses the header and checks the table against it. No GPU, no library
load, no compile.
"""
import ctypes
import re
from pathlib import Path

from kubeflow_amd.ops import _backend

HEADER = (Path(_backend.__file__).resolve().parent / "csrc" / "kf_ops.h")

# Names allowed on one side only, each with its reason. Empty: the table
# configures every exported entry point, including the two that only
# scripts/attn_ablate.py and scripts/probe_tr16.py call.
HEADER_ONLY: dict[str, str] = {}
TABLE_ONLY: dict[str, str] = {}

_PROTO = re.compile(
    r"KF_EXPORT\s+(int64_t|int)\s+(kf_\w+)\s*\(([^)]*)\)\s*;")


def _c_class(param: str) -> str:
    """ABI class of one C parameter declaration: ptr, i64, i32 or f32."""
    if "*" in param:
        return "ptr"
    words = param.replace("const", " ").split()
    assert len(words) == 2, f"parameter needs a type and a name: {param!r}"
    return {"int64_t": "i64", "int": "i32", "float": "f32"}[words[0]]


def _ctypes_class(t) -> str:
    if t is ctypes.c_void_p or issubclass(t, ctypes._Pointer):
        return "ptr"
    return {ctypes.c_int64: "i64", ctypes.c_int32: "i32",
            ctypes.c_float: "f32"}[t]


def parse_header(text: str):
    """name -> (return class, [parameter classes])"""
    text = re.sub(r"//[^\n]*", "", text)
    protos = {}
    for ret, name, params in _PROTO.findall(text):
        assert name not in protos, f"{name} declared twice"
        protos[name] = ({"int": "i32", "int64_t": "i64"}[ret],
                        [_c_class(p) for p in params.split(",")])
    return protos


def table_classes(signatures=None):
    signatures = _backend.SIGNATURES if signatures is None else signatures
    return {
        name: ("i64" if name in _backend._RETURNS_INT64 else "i32",
               [_ctypes_class(t) for t in args])
        for name, args in signatures.items()}


def mismatches(protos, table):
    """Human-readable list of every disagreement between the two sides."""
    out = []
    for name in sorted(set(protos) - set(table) - set(HEADER_ONLY)):
        out.append(f"{name}: in kf_ops.h, not in _backend.SIGNATURES")
    for name in sorted(set(table) - set(protos) - set(TABLE_ONLY)):
        out.append(f"{name}: in _backend.SIGNATURES, not in kf_ops.h")
    for name in sorted(set(protos) & set(table)):
        (cret, cargs), (pret, pargs) = protos[name], table[name]
        if cret != pret:
            out.append(f"{name}: returns {cret} in C, {pret} in ctypes")
        if len(cargs) != len(pargs):
            out.append(f"{name}: {len(cargs)} parameters in C, "
                       f"{len(pargs)} in ctypes")
            continue
        for i, (c, p) in enumerate(zip(cargs, pargs)):
            if c != p:
                out.append(f"{name}: parameter {i} is {c} in C, {p} in ctypes")
    return out


def test_header_parses_every_export():
    text = HEADER.read_text()
    protos = parse_header(text)
    # every KF_EXPORT in the header (bar the #define itself) is a prototype
    # the regex understood
    n_export = len(re.findall(r"^KF_EXPORT\b", text, flags=re.M))
    assert n_export == len(protos) and n_export > 30


def test_table_matches_header():
    assert mismatches(parse_header(HEADER.read_text()), table_classes()) == []


def test_exceptions_are_real():
    protos, table = parse_header(HEADER.read_text()), table_classes()
    assert all(n in protos and n not in table for n in HEADER_ONLY)
    assert all(n in table and n not in protos for n in TABLE_ONLY)


def test_checker_catches_a_dropped_argument_and_a_wrong_class():
    protos = parse_header(HEADER.read_text())
    sigs = dict(_backend.SIGNATURES)
    sigs["kf_rope"] = sigs["kf_rope"][:-1]
    assert mismatches(protos, table_classes(sigs)) == [
        "kf_rope: 15 parameters in C, 14 in ctypes"]
    sigs = dict(_backend.SIGNATURES)
    swapped = list(sigs["kf_swiglu_fwd"])
    swapped[2] = ctypes.c_float
    sigs["kf_swiglu_fwd"] = swapped
    assert mismatches(protos, table_classes(sigs)) == [
        "kf_swiglu_fwd: parameter 2 is i64 in C, f32 in ctypes"]
    del sigs["kf_swiglu_fwd"]
    assert mismatches(protos, table_classes(sigs)) == [
        "kf_swiglu_fwd: in kf_ops.h, not in _backend.SIGNATURES"]


def test_every_kernel_file_sees_the_header():
    """kf_common.h includes kf_ops.h and every .hip file includes kf_common.h
    (directly or through kf_attn_common.h), so a definition that disagrees
    with its prototype cannot compile; and no entry point is re-declared by
    hand anywhere else."""
    csrc = HEADER.parent
    assert '#include "kf_ops.h"' in (csrc / "kf_common.h").read_text()
    assert '#include "kf_common.h"' in (csrc / "kf_attn_common.h").read_text()
    protos = parse_header(HEADER.read_text())
    defined = set()
    for src in sorted(csrc.glob("*.hip")):
        text = src.read_text()
        assert ('#include "kf_common.h"' in text
                or '#include "kf_attn_common.h"' in text), src.name
        assert 'extern "C"' not in text, src.name
        for name in re.findall(
                r"^KF_EXPORT\s+(?:int64_t|int)\s+(kf_\w+)\s*\(", text,
                flags=re.M):
            assert name not in defined, f"{name} defined twice"
            defined.add(name)
    assert defined == set(protos)
