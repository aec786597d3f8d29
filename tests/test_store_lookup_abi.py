"""CPU: the lookup's ABI (include/drp.h "lookup"): the two entry points are declared, exported and
bound, drp_lookup has the header's layout and the constants their values, and every DRP_E_INVAL case
that needs no device is reported before the ctx is touched (the ctx passed here is never followed)."""
import ctypes as C
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "drp.h")
sys.path.insert(0, os.path.join(ROOT, "dat-replication-protocol_amd", "python"))

NEW = ["drp_store_lookup_device", "drp_store_lookup_staged"]
FIELDS = ["flags", "emit_mask", "verdict", "hit_row", "counts", "lack_type", "out_rows", "out_query", "n_out", "rows_cap",
          "reserved", "reserved2"]


def test_declared_exported_and_bound():
    import drp_amd
    src = open(HDR).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", drp_amd.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in NEW:
        assert re.search(r"^int %s\(" % name, src, re.M), name
        assert name in exported, name
        assert name in drp_amd.EXPORTS, name
        fn = getattr(drp_amd.lib(), name)
        assert fn.argtypes is not None and fn.restype is C.c_int, name
    head = src[:src.index("#ifndef DRP_H")]
    assert "drp_store_lookup_device / drp_store_lookup_staged" in head  # the list at the header's top
    for name in ["store_lookup_device", "store_lookup_staged"]:
        assert callable(getattr(drp_amd.Ctx, name)), name
    for name in ["lookup", "get", "sync_reply"]:
        assert callable(getattr(drp_amd.Store, name)), name


def test_abi_version_unchanged():
    import drp_amd
    assert re.search(r"#define DRP_ABI_VERSION (\d+)", open(HDR).read()).group(1) == "5"
    assert drp_amd.lib().drp_abi_version() == 5


def test_lookup_struct_layout():
    """88 bytes; the fields in the header's order, each at the offset the C struct gives it."""
    import drp_amd
    body = re.search(r"typedef struct drp_lookup \{(.*?)\} drp_lookup;", open(HDR).read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.search(r"(\w+)$", decl.strip()).group(1) for decl in body.split(";") if decl.strip()]
    assert names == FIELDS
    K = drp_amd.Lookup
    assert [k for k, _ in K._fields_] == names
    assert C.sizeof(K) == 88
    assert [getattr(K, k).offset for k in names] == [0, 4, 8, 16, 24, 32, 40, 48, 56, 64, 72, 80]


def test_constants():
    import drp_amd
    src = open(HDR).read()
    consts = {k: int(v, 0) for k, v in re.findall(r"#define (DRP_LOOKUP_[A-Z_]+)\s+(0x[0-9a-fA-F]+|\d+)u?\b", src)}
    assert consts == {"DRP_LOOKUP_NONE": 0, "DRP_LOOKUP_ABSENT": 1, "DRP_LOOKUP_BEHIND": 2, "DRP_LOOKUP_LEVEL": 3,
                      "DRP_LOOKUP_AHEAD": 4, "DRP_LOOKUP_REPLY_LACK": 0x100}
    assert re.search(r"#define DRP_LOOKUP_BIT\(code\) \(1u << \(code\)\)", src)
    assert (drp_amd.LOOKUP_NONE, drp_amd.LOOKUP_ABSENT, drp_amd.LOOKUP_BEHIND, drp_amd.LOOKUP_LEVEL,
            drp_amd.LOOKUP_AHEAD, drp_amd.LOOKUP_REPLY_LACK) == (0, 1, 2, 3, 4, 0x100)
    assert [drp_amd.lookup_bit(c) for c in range(5)] == [1, 2, 4, 8, 16]
    assert drp_amd.LOOKUP_FOUND == 4 | 8 | 16


def _call(ctx, store, lk, frames=True):
    import drp_amd
    fr, co = drp_amd.Frames(), drp_amd.Changes()
    return drp_amd.lib().drp_store_lookup_device(ctx, store, None, 0, C.byref(fr) if frames else None, C.byref(co), 0,
                                                 None, lk)


def _fake_ctx():
    """A ctx pointer that must never be followed: it points nowhere."""
    return C.c_void_p(16)


def test_null_ctx_store_and_lookup_are_invalid():
    import drp_amd
    st, lk = drp_amd.StoreDesc(), drp_amd.Lookup()
    assert _call(None, C.byref(st), C.byref(lk)) == drp_amd.DRP_E_INVAL
    assert _call(_fake_ctx(), None, C.byref(lk)) == drp_amd.DRP_E_INVAL
    assert _call(_fake_ctx(), C.byref(st), None) == drp_amd.DRP_E_INVAL
    assert _call(_fake_ctx(), C.byref(st), C.byref(lk), frames=False) == drp_amd.DRP_E_INVAL
    w, n = C.c_uint64(), C.c_uint64()
    L = drp_amd.lib()
    assert L.drp_store_lookup_staged(None, C.byref(st), None, 0, None, 0, C.byref(w), C.byref(n), None) == drp_amd.DRP_E_INVAL
    assert L.drp_store_lookup_staged(_fake_ctx(), None, None, 0, None, 0, C.byref(w), C.byref(n), None) == drp_amd.DRP_E_INVAL
    # a reply that is neither an emit_mask nor DRP_LOOKUP_REPLY_LACK alone
    for reply in [1, 2, 32, 0x100 | 4, 0x200]:
        assert L.drp_store_lookup_staged(_fake_ctx(), C.byref(st), None, reply, None, 0, C.byref(w), C.byref(n),
                                         None) == drp_amd.DRP_E_INVAL, reply


def _valid_store(keep):
    """A drp_store whose every pointer is set (to host memory nobody reads) and max_keys = 4: with it
    a call gets past the store's own checks, so DRP_E_INVAL below comes from the drp_lookup."""
    import drp_amd
    buf = C.create_string_buffer(256)
    keep.append(buf)
    p = C.addressof(buf)
    p += -p % 16
    fr = drp_amd.Frames(p, p + 16, p + 32)
    co = drp_amd.Changes(*([p + 48] * 10), None)
    return drp_amd.StoreDesc(p, 64, fr, co, 4, p + 64, p + 128, 0), p + 32


def test_bad_lookup_fields_are_invalid_without_a_device():
    """Unknown flags; an emit_mask with the NONE or ABSENT bit or a bit above 4; out_rows without
    n_out; with rows_cap > 0 a NULL array in out_rows; lack_type aliasing the store's type column.
    The store is complete, so these are the drp_lookup's own cases, and the ctx is never followed."""
    import drp_amd
    keep = []
    st, type_p = _valid_store(keep)
    bad = []
    for flags in [1, 2, 0x80000000]:
        bad.append(drp_amd.Lookup(flags=flags))
    for mask in [1, 2, 1 | 4, 2 | 16, 32, 64, 0x100, 0x80000000, 0xFFFFFFFF]:
        bad.append(drp_amd.Lookup(emit_mask=mask))
    rows = drp_amd.ChangeSrc(*([type_p] * 10))
    bad.append(drp_amd.Lookup(emit_mask=4, out_rows=C.pointer(rows), rows_cap=0))             # no n_out
    hole = drp_amd.ChangeSrc(*([type_p] * 9), None)
    bad.append(drp_amd.Lookup(emit_mask=4, out_rows=C.pointer(hole), n_out=type_p, rows_cap=1))  # a NULL array
    bad.append(drp_amd.Lookup(lack_type=type_p))                                               # aliasing
    for lk in bad:
        assert _call(_fake_ctx(), C.byref(st), C.byref(lk)) == drp_amd.DRP_E_INVAL
