"""CPU: the refined-digest entry points are declared, exported and bound; DRP_DIGEST_MAX_SUB_BITS; the
ABI version did not move (symbols were only added); NULL and out-of-range arguments are rejected without
a device."""
import ctypes as C
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "drp.h")
sys.path.insert(0, os.path.join(ROOT, "dat-replication-protocol_amd", "python"))

NAMES = ["drp_digest_refine_device", "drp_digest_diff_cells_device", "drp_select_refined_device"]


def test_header_declares_the_refined_entry_points():
    src = open(HDR).read()
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, src, re.M), name
    assert int(re.search(r"#define DRP_ABI_VERSION (\d+)", src).group(1)) == 5  # symbols were only added
    assert int(re.search(r"#define DRP_DIGEST_MAX_BITS (\d+)", src).group(1)) == 16
    assert int(re.search(r"#define DRP_DIGEST_MAX_SUB_BITS (\d+)", src).group(1)) == 8
    # the opening comment lists them, with no reference counterpart
    head = src[:src.index("#ifndef DRP_H")]
    at = head.index(" / ".join(NAMES))
    assert "no reference counterpart" in head[at:at + 300]
    import drp_amd
    assert drp_amd.lib().drp_abi_version() == 5
    assert drp_amd.DIGEST_MAX_SUB_BITS == 8 and drp_amd.DIGEST_MAX_BITS == 16
    for name in NAMES:
        assert name in drp_amd.EXPORTS, name
    for method in ["digest_refine_device", "digest_diff_cells_device", "select_refined_device"]:
        assert callable(getattr(drp_amd.Ctx, method))
    assert callable(drp_amd.Store.digest_refined) and callable(drp_amd.Store.reconcile_refined)


def test_library_exports_them():
    import drp_amd
    L = C.CDLL(drp_amd.LIB_PATH)
    for name in NAMES:
        assert L[name] is not None, name  # (a symbol the library does not export raises AttributeError)


def test_invalid_arguments_without_a_device():
    import drp_amd
    L = drp_amd.lib()
    fr, co, rows = drp_amd.Frames(), drp_amd.Changes(), drp_amd.ChangeSrc()
    fake = C.c_void_p(16)  # never dereferenced: the arguments are checked first
    E = drp_amd.DRP_E_INVAL

    def refine(ctx=fake, wire=None, nbytes=0, frames=C.byref(fr), cols=C.byref(co), n=0, flt=None, bits=0, bset=fake,
               sub_bits=1, cells2=fake, cap=2, totals=fake):
        return L.drp_digest_refine_device(ctx, wire, nbytes, frames, cols, n, flt, bits, bset, sub_bits, cells2, cap,
                                          totals)

    assert refine(ctx=None) == E
    assert refine(frames=None) == E
    assert refine(cols=None) == E
    assert refine(nbytes=8) == E  # a NULL wire with bytes in it
    assert refine(wire=fake, nbytes=8, n=1) == E  # NULL columns
    assert refine(bits=17) == E
    assert refine(sub_bits=0) == E
    assert refine(sub_bits=9) == E
    assert refine(bset=None) == E
    assert refine(cells2=None) == E
    assert refine(totals=None) == E
    assert refine(flt=C.byref(drp_amd.make_filter(flags=0x100))) == E

    most = 65536 << 8
    for a in [(None, fake, fake, 1, fake, fake), (fake, None, fake, 1, fake, fake), (fake, fake, None, 1, fake, fake),
              (fake, fake, fake, 1, None, fake), (fake, fake, fake, 1, fake, None), (fake, fake, fake, most + 1, fake, fake),
              (fake, fake, fake, 1 << 40, fake, fake)]:
        assert L.drp_digest_diff_cells_device(*a) == E, a

    def sel(ctx=fake, bits=0, bset=fake, sub_bits=1, cset=fake, out=C.byref(rows), nsel=fake, flt=None):
        return L.drp_select_refined_device(ctx, None, 0, C.byref(fr), C.byref(co), 0, flt, bits, bset, sub_bits, cset,
                                           out, None, nsel)

    assert sel(ctx=None) == E
    assert sel(bits=17) == E
    assert sel(sub_bits=0) == E
    assert sel(sub_bits=9) == E
    assert sel(bset=None) == E
    assert sel(cset=None) == E
    assert sel(out=None) == E
    assert sel(nsel=None) == E
    assert sel(flt=C.byref(drp_amd.make_filter(flags=0x100))) == E
