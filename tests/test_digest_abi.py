"""CPU: the digest entry points are declared, exported and bound; the cell's layout; the LDS threshold
the binding names is the kernels'; NULL arguments are rejected without a device."""
import ctypes as C
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "drp.h")
KERNELS_H = os.path.join(ROOT, "dat-replication-protocol_amd", "csrc", "drp_kernels.h")
sys.path.insert(0, os.path.join(ROOT, "dat-replication-protocol_amd", "python"))

NAMES = ["drp_digest_device", "drp_digest_diff_device", "drp_select_buckets_device"]


def test_header_declares_the_digest_entry_points():
    src = open(HDR).read()
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, src, re.M), name
    assert int(re.search(r"#define DRP_ABI_VERSION (\d+)", src).group(1)) == 5  # symbols were only added
    assert int(re.search(r"#define DRP_DIGEST_MAX_BITS (\d+)", src).group(1)) == 16
    import drp_amd
    assert drp_amd.lib().drp_abi_version() == 5
    for name in NAMES:
        assert name in drp_amd.EXPORTS, name
    for method in ["digest_device", "digest_diff_device", "select_buckets_device"]:
        assert callable(getattr(drp_amd.Ctx, method))
    assert callable(drp_amd.Store.digest) and callable(drp_amd.Store.reconcile)


def test_library_exports_them():
    import drp_amd
    L = C.CDLL(drp_amd.LIB_PATH)
    for name in NAMES:
        assert L[name] is not None, name  # (a symbol the library does not export raises AttributeError)


def test_cell_layout_and_constants():
    import drp_amd
    assert C.sizeof(drp_amd.DigestCell) == 16
    assert [k for k, _ in drp_amd.DigestCell._fields_] == ["count", "sum"]
    src = open(HDR).read()
    body = re.search(r"typedef struct drp_digest_cell \{(.*?)\} drp_digest_cell;", src, re.S).group(1)
    assert [f.strip() for f in re.search(r"uint64_t ([^;]*);", body).group(1).split(",")] == ["count", "sum"]
    assert drp_amd.DIGEST_MAX_BITS == 16
    lds = int(re.search(r"constexpr uint32_t DIG_LDS_BITS = (\d+);", open(KERNELS_H).read()).group(1))
    assert drp_amd.DIGEST_LDS_BITS == lds and 0 < lds < 16


def test_null_arguments_are_invalid_without_a_device():
    import drp_amd
    L = drp_amd.lib()
    fr, co, rows = drp_amd.Frames(), drp_amd.Changes(), drp_amd.ChangeSrc()
    fake = C.c_void_p(16)  # never dereferenced: the arguments are checked first
    E = drp_amd.DRP_E_INVAL
    # NULL ctx, NULL frames / cols, NULL cells, bits > 16, a NULL wire with bytes in it
    assert L.drp_digest_device(None, None, 0, C.byref(fr), C.byref(co), 0, None, 0, fake, None) == E
    assert L.drp_digest_device(fake, None, 0, None, C.byref(co), 0, None, 0, fake, None) == E
    assert L.drp_digest_device(fake, None, 0, C.byref(fr), None, 0, None, 0, fake, None) == E
    assert L.drp_digest_device(fake, None, 0, C.byref(fr), C.byref(co), 0, None, 0, None, None) == E
    assert L.drp_digest_device(fake, None, 0, C.byref(fr), C.byref(co), 0, None, 17, fake, None) == E
    assert L.drp_digest_device(fake, None, 8, C.byref(fr), C.byref(co), 0, None, 0, fake, None) == E
    assert L.drp_digest_device(fake, fake, 8, C.byref(fr), C.byref(co), 1, None, 0, fake, None) == E  # NULL columns
    bad = drp_amd.make_filter(flags=0x100)
    assert L.drp_digest_device(fake, None, 0, C.byref(fr), C.byref(co), 0, C.byref(bad), 0, fake, None) == E
    for a in [(None, fake, fake, 0, fake, fake), (fake, None, fake, 0, fake, fake), (fake, fake, None, 0, fake, fake),
              (fake, fake, fake, 0, None, fake), (fake, fake, fake, 0, fake, None), (fake, fake, fake, 17, fake, fake)]:
        assert L.drp_digest_diff_device(*a) == E, a
    sel = lambda ctx, bits, bset, out, nsel: L.drp_select_buckets_device(ctx, None, 0, C.byref(fr), C.byref(co), 0, None,
                                                                         bits, bset, out, None, nsel)
    assert sel(None, 0, fake, C.byref(rows), fake) == E
    assert sel(fake, 17, fake, C.byref(rows), fake) == E
    assert sel(fake, 0, None, C.byref(rows), fake) == E
    assert sel(fake, 0, fake, None, fake) == E
    assert sel(fake, 0, fake, C.byref(rows), None) == E
