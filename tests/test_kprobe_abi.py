"""(CPU) The ctypes table of tests/kprobe/__init__.py against the C entry
points of tests/kprobe/vs_kprobe.cpp: same names, same argument counts, and
integer widths that match (a uint64_t pointer declared c_uint32 would
truncate a device address without any error)."""
import os
import re

import kprobe

SRC = os.path.join(os.path.dirname(os.path.abspath(kprobe.__file__)), "vs_kprobe.cpp")
CTYPE = {"uint64_t": kprobe.u64, "uint32_t": kprobe.u32, "int": kprobe.i32, "double": kprobe.f64,
         "uint32_t*": kprobe.pu32}


def _entry_points():
    text = open(SRC).read()
    text = text[text.index('extern "C"'):]
    out = {}
    for m in re.finditer(r"^(\w+)\s+kp_(\w+)\(([^)]*)\)\s*\{", text, re.M | re.S):
        args = [a.strip() for a in m.group(3).split(",") if a.strip()]
        types = []
        for a in args:
            ty = a.rsplit(" ", 1)[0].replace(" ", "")
            types.append(ty)
        out[m.group(2)] = (m.group(1), types)
    return out


def test_every_entry_point_is_declared_with_matching_types():
    eps = _entry_points()
    declared = set(kprobe._SIGS) | set(kprobe._CONSTS64) | set(kprobe._CONSTS32)
    assert set(eps) == declared, set(eps) ^ declared
    for name, (res, args) in kprobe._SIGS.items():
        cres, cargs = eps[name]
        assert [CTYPE[t] for t in cargs] == list(args), name
        assert (None if cres == "void" else CTYPE[cres]) == res, name
    for name in kprobe._CONSTS64:
        assert eps[name] == ("uint64_t", []), name
    for name in kprobe._CONSTS32:
        assert eps[name] == ("uint32_t", []), name
