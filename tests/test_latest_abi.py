"""CPU: the latest-per-key entry points are declared, exported and bound, and reject a NULL ctx
without a device."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "drp.h")
sys.path.insert(0, os.path.join(ROOT, "dat-replication-protocol_amd", "python"))

NAMES = ["drp_latest_device", "drp_latest_staged", "drp_set_latest_hash_mask"]


def test_header_declares_the_latest_entry_points():
    src = open(HDR).read()
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, src, re.M), name
    assert int(re.search(r"#define DRP_ABI_VERSION (\d+)", src).group(1)) == 5  # symbols were only added
    import drp_amd
    for name in NAMES:
        assert name in drp_amd.EXPORTS, name
    for method in ["latest_device", "latest_staged", "set_latest_hash_mask"]:
        assert callable(getattr(drp_amd.Ctx, method))


def test_null_ctx_is_invalid_without_a_device():
    import drp_amd
    L = drp_amd.lib()
    assert L.drp_latest_device(None, None, 0, None, None, 0, None, None, None, None) == drp_amd.DRP_E_INVAL
    assert L.drp_latest_staged(None, None, None, 0, None, None) == drp_amd.DRP_E_INVAL
    assert L.drp_set_latest_hash_mask(None, 0) == drp_amd.DRP_E_INVAL
