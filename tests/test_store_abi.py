"""CPU: the store's entry points are declared, exported and bound; drp_store_table_bytes' values; the
layout of the two structs; a NULL ctx or store is rejected without a device."""
import ctypes as C
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "drp.h")
sys.path.insert(0, os.path.join(ROOT, "dat-replication-protocol_amd", "python"))

INT_NAMES = ["drp_store_init", "drp_store_merge_device", "drp_store_merge_staged", "drp_store_compact",
             "drp_store_query"]


def test_header_declares_the_store_entry_points():
    src = open(HDR).read()
    for name in INT_NAMES:
        assert re.search(r"^int %s\(" % name, src, re.M), name
    assert re.search(r"^uint64_t drp_store_table_bytes\(", src, re.M)
    assert int(re.search(r"#define DRP_ABI_VERSION (\d+)", src).group(1)) == 5  # symbols were only added
    import drp_amd
    for name in INT_NAMES + ["drp_store_table_bytes"]:
        assert name in drp_amd.EXPORTS, name
    for method in ["store_init", "store_merge_device", "store_merge_staged", "store_compact", "store_query"]:
        assert callable(getattr(drp_amd.Ctx, method))
    assert callable(drp_amd.Store.fanout)


@pytest.mark.parametrize("max_keys,want", [(1, 16), (3, 64), (1024, 16384), (0, 0), (2**31 + 1, 0), (2**31, 8 * 2**32)])
def test_table_bytes(max_keys, want):
    import drp_amd
    assert drp_amd.lib().drp_store_table_bytes(max_keys) == want


def test_struct_sizes():
    import drp_amd
    assert C.sizeof(drp_amd.StoreInfo) == 112
    assert C.sizeof(drp_amd.StoreDesc) == 160
    src = open(HDR).read()
    body = re.search(r"typedef struct drp_store_info \{(.*?)\} drp_store_info;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip() for decl in re.findall(r"uint64_t ([^;]*);", body) for f in decl.split(",")]
    assert fields == [k for k, _ in drp_amd.StoreInfo._fields_]
    assert fields[:13] == ["rows", "arena_used", "arena_dead", "merges", "winners", "inserted", "replaced", "unchanged",
                           "stale", "skipped", "refused", "need_rows", "need_bytes"]


def test_null_arguments_are_invalid_without_a_device():
    import drp_amd
    L = drp_amd.lib()
    s = drp_amd.StoreDesc()
    info = drp_amd.StoreInfo()
    fake = C.c_void_p(16)  # never dereferenced: the store is checked first
    for ctx, st in [(None, C.byref(s)), (fake, None), (None, None)]:
        assert L.drp_store_init(ctx, st) == drp_amd.DRP_E_INVAL
        assert L.drp_store_merge_device(ctx, st, None, 0, None, None, 0, None) == drp_amd.DRP_E_INVAL
        assert L.drp_store_merge_staged(ctx, st, None, C.byref(info)) == drp_amd.DRP_E_INVAL
        assert L.drp_store_compact(ctx, st, None, 0) == drp_amd.DRP_E_INVAL
        assert L.drp_store_query(ctx, st, C.byref(info)) == drp_amd.DRP_E_INVAL
