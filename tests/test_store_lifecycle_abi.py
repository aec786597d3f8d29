"""CPU: the store lifecycle's ABI (include/drp.h "store lifecycle"): the two entry points are declared,
exported, covered by csrc/libdrp.map and bound, the ABI version is unchanged, every DRP_E_INVAL case
that needs no device is reported before the ctx is touched (the ctx passed here is never followed),
and the Python layer has the calls on top of them."""
import ctypes as C
import fnmatch
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "drp.h")
MAP = os.path.join(ROOT, "dat-replication-protocol_amd", "csrc", "libdrp.map")
sys.path.insert(0, os.path.join(ROOT, "dat-replication-protocol_amd", "python"))

NEW = ["drp_store_load_device", "drp_store_rehash_device"]


def test_declared_exported_listed_and_bound():
    import drp_amd
    src = open(HDR).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", drp_amd.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    globs = re.search(r"global:(.*?)local:", open(MAP).read(), re.S).group(1)
    patterns = [p.strip() for p in globs.split(";") if p.strip()]
    for name in NEW:
        assert re.search(r"^int %s\(" % name, src, re.M), name
        assert name in exported, name
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), (name, patterns)
        assert name in drp_amd.EXPORTS, name
        fn = getattr(drp_amd.lib(), name)
        assert fn.argtypes is not None and fn.restype is C.c_int, name
    assert len(drp_amd.lib().drp_store_load_device.argtypes) == 9
    assert len(drp_amd.lib().drp_store_rehash_device.argtypes) == 3
    head = src[:src.index("#ifndef DRP_H")]
    assert "drp_store_load_device / drp_store_rehash_device" in head  # the list at the header's top
    assert "/* ---- store lifecycle" in src
    for name in ["store_load_device", "store_rehash_device"]:
        assert callable(getattr(drp_amd.Ctx, name)), name


def test_abi_version_unchanged():
    import drp_amd
    assert re.search(r"#define DRP_ABI_VERSION (\d+)", open(HDR).read()).group(1) == "5"  # symbols were only added
    assert drp_amd.lib().drp_abi_version() == 5


def test_store_methods_exist():
    import drp_amd
    for name in ["grow", "retain", "state"]:
        assert callable(getattr(drp_amd.Store, name)), name
    assert isinstance(drp_amd.Store.__dict__["from_state"], classmethod)


def _valid_store(keep):
    """A drp_store whose every pointer is set (to host memory nobody reads) and max_keys = 4."""
    import drp_amd
    buf = C.create_string_buffer(256)
    keep.append(buf)
    p = C.addressof(buf)
    p += -p % 16
    fr = drp_amd.Frames(p, p + 16, p + 32)
    co = drp_amd.Changes(*([p + 48] * 10), None)
    return drp_amd.StoreDesc(p, 64, fr, co, 4, p + 64, p + 128, 0)


def test_null_and_incomplete_arguments_are_invalid_without_a_device():
    import drp_amd
    L = drp_amd.lib()
    empty = drp_amd.StoreDesc()
    fr, co = drp_amd.Frames(), drp_amd.Changes()
    fake = C.c_void_p(16)  # never dereferenced: the arguments are checked first
    for ctx, st in [(None, C.byref(empty)), (fake, None), (None, None), (fake, C.byref(empty))]:
        assert L.drp_store_load_device(ctx, st, None, 0, C.byref(fr), C.byref(co), 0, None, None) == drp_amd.DRP_E_INVAL
        assert L.drp_store_rehash_device(ctx, st, None) == drp_amd.DRP_E_INVAL
    keep = []
    st = _valid_store(keep)
    assert L.drp_store_load_device(None, C.byref(st), None, 0, C.byref(fr), C.byref(co), 0, None, None) == drp_amd.DRP_E_INVAL
    assert L.drp_store_rehash_device(None, C.byref(st), None) == drp_amd.DRP_E_INVAL
    # drp_store_merge_device's cases: no frames, no cols, bytes NULL with nbytes > 0
    assert L.drp_store_load_device(fake, C.byref(st), None, 0, None, C.byref(co), 0, None, None) == drp_amd.DRP_E_INVAL
    assert L.drp_store_load_device(fake, C.byref(st), None, 0, C.byref(fr), None, 0, None, None) == drp_amd.DRP_E_INVAL
    assert L.drp_store_load_device(fake, C.byref(st), None, 8, C.byref(fr), C.byref(co), 0, None, None) == drp_amd.DRP_E_INVAL
    # a misaligned arena, max_keys out of range
    for field, value in [("arena", st.arena + 8), ("max_keys", 0), ("max_keys", 2**31 + 1), ("table", None)]:
        bad = _valid_store(keep)
        setattr(bad, field, value)
        assert L.drp_store_rehash_device(fake, C.byref(bad), None) == drp_amd.DRP_E_INVAL, field
        assert L.drp_store_load_device(fake, C.byref(bad), None, 0, C.byref(fr), C.byref(co), 0, None,
                                       None) == drp_amd.DRP_E_INVAL, field
