"""CPU: the binding's signature table states every declaration of include/drp.h: as many argtypes as
the header has parameters, and the restype of the declared return type."""
import ctypes as C
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "drp.h")
sys.path.insert(0, os.path.join(ROOT, "dat-replication-protocol_amd", "python"))

RESTYPES = {"int": C.c_int, "void": None, "void *": C.c_void_p, "uint64_t": C.c_uint64}


def declarations():
    """{name: (return type, [parameter, ...])} of every drp_* function the header declares."""
    src = re.sub(r"/\*.*?\*/", " ", open(HDR).read(), flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    out = {}
    for ret, star, name, params in re.findall(r"^\s*(int|void|uint64_t)\s*(\*?)\s*(drp_\w+)\(([^)]*)\)\s*;", src, re.M):
        params = [p.strip() for p in params.split(",")]
        out[name] = (ret + (" *" if star else ""), [] if params == ["void"] else params)
    return out


DECL = declarations()


def test_the_parse_sees_the_whole_header():
    assert len(DECL) == len(re.findall(r"^(?:int|void|uint64_t)\s*\*?\s*drp_\w+\(", open(HDR).read(), re.M)) >= 60
    assert DECL["drp_abi_version"] == ("int", [])
    assert DECL["drp_stream"][0] == "void *" and DECL["drp_close"][0] == "void"
    assert DECL["drp_store_table_bytes"] == ("uint64_t", ["uint64_t max_keys"])
    assert len(DECL["drp_store_lookup_staged"][1]) == 9  # (a comment inside the parameter list)
    assert all(p and p != "void" for _, ps in DECL.values() for p in ps)


def test_the_table_is_the_header():
    import drp_amd
    assert set(drp_amd.SIGNATURES) == set(DECL) and sorted(drp_amd.EXPORTS) == sorted(DECL)


@pytest.mark.parametrize("name", sorted(DECL))
def test_signature(name):
    import drp_amd
    ret, params = DECL[name]
    fn = getattr(drp_amd.lib(), name)
    assert fn.argtypes is not None and len(fn.argtypes) == len(params), (name, fn.argtypes, params)
    assert fn.restype is RESTYPES[ret], (name, fn.restype, ret)


def test_staged_fanout_arities():
    import drp_amd
    L = drp_amd.lib()
    assert len(L.drp_fanout_latest_staged.argtypes) == 7
    assert len(L.drp_fanout_news_staged.argtypes) == 11
