"""CPU: the C-ABI library loads and exports every symbol include/sequitr_hip.h declares
(no compute calls -- there is no GPU here), and the host-side checks fail loudly."""
import os
import re

import numpy as np
import pytest
import torch

from sequitr_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    src = open(os.path.join(ROOT, "include", "sequitr_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(sq_[A-Za-z0-9_]+)\s*\(", src)))


def test_header_symbols_all_bound_and_exported():
    names = _declared_symbols()
    assert len(names) >= 13
    lib = _lib.load()
    for n in names:
        assert n in _lib.SIGNATURES, "header declares %s but _lib.SIGNATURES does not bind it" % n
        assert hasattr(lib, n), "libsequitr_hip.so does not export %s" % n
    assert set(_lib.SIGNATURES) == set(names)
    assert lib.sq_version() >= 100


def _prototypes():
    """{name: (return kind, [argument kinds])} of every prototype of the header; a kind is 'ptr', 'int', 'int64', 'uint32',
    'float' or 'double'"""
    src = open(os.path.join(ROOT, "include", "sequitr_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    src = re.sub(r"^\s*#[^\n]*", "", src, flags=re.M)

    def kind(decl):
        decl = " ".join(decl.replace("*", " * ").split())
        if "*" in decl:
            return "ptr"
        scalars = {"int": "int", "int32_t": "int", "int64_t": "int64", "uint32_t": "uint32", "unsigned": "uint32",
                   "float": "float", "double": "double"}
        assert decl in scalars, "a type the ABI test does not know: %r" % decl
        return scalars[decl]

    protos = {}
    for ret, name, args in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(sq_[A-Za-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        assert name not in protos, "%s is declared twice" % name
        args = [] if args.strip() in ("", "void") else args.split(",")
        # `type *name`: the name is the last word, whatever stands before it is the type
        protos[name] = (kind(ret), [kind(re.sub(r"\b\w+\s*$", "", a)) for a in args])
    return protos


def _ctypes_kind(t):
    import ctypes
    if t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer)):
        return "ptr"
    kinds = {ctypes.c_int: "int", ctypes.c_int32: "int", ctypes.c_int64: "int64", ctypes.c_uint32: "uint32",
             ctypes.c_float: "float", ctypes.c_double: "double"}
    assert t in kinds, "a ctypes type the ABI test does not know: %r" % (t,)
    return kinds[t]


def signature_mismatches(signatures):
    """every difference between the header's prototypes and a SIGNATURES table, one message per entry"""
    bad = []
    for name, (ret, args) in sorted(_prototypes().items()):
        if name not in signatures:
            bad.append("%s: not in SIGNATURES" % name)
            continue
        res, argtypes = signatures[name]
        got = (_ctypes_kind(res), [_ctypes_kind(t) for t in argtypes])
        if got[0] != ret:
            bad.append("%s: returns %s in the header, %s in SIGNATURES" % (name, ret, got[0]))
        if len(got[1]) != len(args):
            bad.append("%s: %d arguments in the header, %d in SIGNATURES" % (name, len(args), len(got[1])))
            continue
        bad += ["%s: argument %d is %s in the header, %s in SIGNATURES" % (name, i, a, g)
                for i, (a, g) in enumerate(zip(args, got[1])) if a != g]
    return bad


def test_signatures_match_the_prototypes_argument_by_argument():
    """a c_int where the header says int64_t, or a c_float for a double, passes garbage and raises nothing"""
    protos = _prototypes()
    assert set(protos) == set(_declared_symbols()) and len(protos) >= 235
    kinds = {k for ret, args in protos.values() for k in [ret] + args}
    assert kinds == {"ptr", "int", "int64", "uint32", "float", "double"}       # the parse tells them all apart
    bad = signature_mismatches(_lib.SIGNATURES)
    assert not bad, "\n".join(bad)


def test_a_wrong_signature_is_named():
    """the comparison itself: one entry narrowed from int64_t to int, one float for a double, one argument dropped"""
    import ctypes
    wrong = dict(_lib.SIGNATURES)
    res, args = wrong["sq_argmax_u8"]
    assert args[2] is ctypes.c_int64
    wrong["sq_argmax_u8"] = (res, args[:2] + [ctypes.c_int] + args[3:])
    res, args = wrong["sq_weightmap_edt_f32"]
    assert args[7] is ctypes.c_double
    wrong["sq_weightmap_edt_f32"] = (res, args[:7] + [ctypes.c_float] + args[8:])
    res, args = wrong["sq_frame_stats"]
    wrong["sq_frame_stats"] = (res, args[:-1])
    assert signature_mismatches(wrong) == [
        "sq_argmax_u8: argument 2 is int64 in the header, int in SIGNATURES",
        "sq_frame_stats: 9 arguments in the header, 8 in SIGNATURES",
        "sq_weightmap_edt_f32: argument 7 is double in the header, float in SIGNATURES"]


def test_host_side_validation_needs_no_gpu():
    lib = _lib.load()
    # NULL pointers are refused before any launch, with a message
    rc = lib.sq_conv2d_nhwc_fwd_f32(None, None, None, None, 1, 16, 16, 16, 16, 3, 1.0, 1, None)
    assert rc == -1 and b"null" in lib.sq_last_error()
    rc = lib.sq_maxpool2x2_fwd_f32(16, 32, 1, 15, 16, 16, None)
    assert rc == -1 and b"even" in lib.sq_last_error()
    rc = lib.sq_convT2x2s2_nhwc_fwd_f32(16, 16, None, None, 16, 1, 4, 4, 12, 16, 0, None)
    assert rc == -1 and b"multiple of 16" in lib.sq_last_error()
    assert lib.sq_wsoftmax_ce_partials(10 ** 9) == 2048 and lib.sq_wsoftmax_ce_partials(100) == 1


def test_no_cpu_fallback():
    x = torch.zeros(1, 16, 16, 16)
    w = torch.zeros(3, 3, 16, 16)
    with pytest.raises(_lib.SequitrHipError):
        ops.conv2d(x, w)


def test_missing_library_is_loud(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libsequitr_hip.so")
    with pytest.raises(_lib.SequitrHipError):
        _lib.load()
