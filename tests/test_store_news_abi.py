"""CPU: the merge report's ABI (include/drp.h "merge report"): the three entry points are declared,
exported and bound, drp_merge_report has the header's layout, the calls reject a NULL ctx or store
before they touch a device, and the Store helper carries the hub step."""
import ctypes as C
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "drp.h")
sys.path.insert(0, os.path.join(ROOT, "dat-replication-protocol_amd", "python"))

NEW = ["drp_store_merge_report_device", "drp_store_merge_news_staged", "drp_fanout_news_staged"]


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


def test_abi_version_unchanged():
    import drp_amd
    assert re.search(r"#define DRP_ABI_VERSION (\d+)", open(HDR).read()).group(1) == "5"
    assert drp_amd.lib().drp_abi_version() == 5


def test_report_struct_layout():
    """64 bytes; the fields in the header's order, each at the offset the C struct gives it."""
    import drp_amd
    body = re.search(r"typedef struct drp_merge_report \{(.*?)\} drp_merge_report;", open(HDR).read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            first, *rest = decl.split(",")
            names += [re.search(r"(\w+)$", first.strip()).group(1)] + [r.strip().lstrip("*") for r in rest]
    assert names == ["flags", "reserved", "outcome", "news_type", "reply_rows", "reply_idx", "n_reply", "reply_cap",
                     "reserved2"]
    R = drp_amd.MergeReport
    assert [k for k, _ in R._fields_] == names
    assert C.sizeof(R) == 64
    assert [getattr(R, k).offset for k in names] == [0, 4, 8, 16, 24, 32, 40, 48, 56]
    consts = dict(re.findall(r"#define (DRP_MERGE_\w+|DRP_REPORT_\w+) (\w+)", open(HDR).read()))
    assert {k: int(v, 0) for k, v in consts.items()} == {
        "DRP_MERGE_NONE": 0, "DRP_MERGE_INSERTED": 1, "DRP_MERGE_REPLACED": 2, "DRP_MERGE_UNCHANGED": 3,
        "DRP_MERGE_STALE": 4, "DRP_MERGE_SKIPPED": 5, "DRP_REPORT_KEEP_BLOBS": 1}
    assert (drp_amd.MERGE_NONE, drp_amd.MERGE_INSERTED, drp_amd.MERGE_REPLACED, drp_amd.MERGE_UNCHANGED,
            drp_amd.MERGE_STALE, drp_amd.MERGE_SKIPPED, drp_amd.REPORT_KEEP_BLOBS) == (0, 1, 2, 3, 4, 5, 1)


def test_null_ctx_and_store_are_invalid():
    """No device is touched: DRP_E_INVAL for a NULL ctx, and for a NULL store behind a ctx pointer
    that is never followed."""
    import drp_amd
    L = drp_amd.lib()
    fr, co, st = drp_amd.Frames(), drp_amd.Changes(), drp_amd.StoreDesc()
    rep, info = drp_amd.MergeReport(), drp_amd.StoreInfo()
    fake = C.c_void_p(C.addressof(C.create_string_buffer(8)))  # (a ctx the NULL-store check never reads)
    for ctx, store in [(None, C.byref(st)), (fake, None)]:
        assert L.drp_store_merge_report_device(ctx, store, None, 0, C.byref(fr), C.byref(co), 0, None,
                                               C.byref(rep)) == drp_amd.DRP_E_INVAL
        assert L.drp_store_merge_news_staged(ctx, store, None, C.byref(info)) == drp_amd.DRP_E_INVAL
    off, nsel = (C.c_uint64 * 2)(), (C.c_uint64 * 1)()
    assert L.drp_fanout_news_staged(None, drp_amd.filter_array([None]), 1, None, 0, off, nsel, None, None, 0,
                                    None) == drp_amd.DRP_E_INVAL


def test_store_methods_exist():
    import drp_amd
    for name in ["merge_report", "relay_news", "reply_bytes"]:
        assert callable(getattr(drp_amd.Store, name)), name
    for name in ["store_merge_report_device", "store_merge_news_staged", "fanout_news_staged"]:
        assert callable(getattr(drp_amd.Ctx, name)), name
