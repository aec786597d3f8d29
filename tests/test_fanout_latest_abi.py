"""CPU: the entry points of the fan-out of latest per key are declared, exported and bound, and
reject a NULL ctx without a device."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "drp.h")
sys.path.insert(0, os.path.join(ROOT, "dat-replication-protocol_amd", "python"))

NAMES = ["drp_fanout_latest_device", "drp_fanout_latest_staged", "drp_set_fanout_latest_pass"]


def test_header_declares_the_fanout_latest_entry_points():
    src = open(HDR).read()
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, src, re.M), name
    assert int(re.search(r"#define DRP_ABI_VERSION (\d+)", src).group(1)) == 5  # symbols were only added
    import drp_amd
    for name in NAMES:
        assert name in drp_amd.EXPORTS, name
    for method in ["fanout_latest_device", "fanout_latest_staged", "set_fanout_latest_pass"]:
        assert callable(getattr(drp_amd.Ctx, method))


def test_null_ctx_is_invalid_without_a_device():
    import drp_amd
    L = drp_amd.lib()
    assert L.drp_abi_version() == 5
    assert L.drp_fanout_latest_device(None, None, 0, None, None, 0, None, 1, None, 0, None,
                                      None) == drp_amd.DRP_E_INVAL
    assert L.drp_fanout_latest_staged(None, None, 1, None, 0, None, None) == drp_amd.DRP_E_INVAL
    assert L.drp_set_fanout_latest_pass(None, 0) == drp_amd.DRP_E_INVAL
