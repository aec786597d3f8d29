"""CPU: the fan-out entry points are declared, exported and bound, reject a NULL ctx without a
device, and the Python structs have the C layout."""
import ctypes as C
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "drp.h")
sys.path.insert(0, os.path.join(ROOT, "dat-replication-protocol_amd", "python"))


def test_header_declares_the_fanout():
    src = open(HDR).read()
    assert re.search(r"^int drp_fanout_device\(", src, re.M) and re.search(r"^int drp_fanout_staged\(", src, re.M)
    assert int(re.search(r"#define DRP_FANOUT_MAX (\d+)", src).group(1)) == 64
    assert int(re.search(r"#define DRP_ABI_VERSION (\d+)", src).group(1)) == 5  # symbols were only added
    import drp_amd
    assert drp_amd.FANOUT_MAX == 64
    assert "drp_fanout_device" in drp_amd.EXPORTS and "drp_fanout_staged" in drp_amd.EXPORTS


def test_null_ctx_is_invalid_without_a_device():
    import drp_amd
    L = drp_amd.lib()
    f = drp_amd.filter_array([None])
    assert L.drp_fanout_device(None, None, 0, None, None, 0, f, 1, None, 0, None, None, None) == drp_amd.DRP_E_INVAL
    assert L.drp_fanout_staged(None, f, 1, None, 0, None, None, None, None, 0, None) == drp_amd.DRP_E_INVAL


def test_struct_sizes_match_the_header(tmp_path):
    """sizeof of the structs the fan-out passes by pointer, from a C program compiled against
    include/drp.h with the host compiler."""
    import drp_amd
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "drp.h"\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(drp_splice), sizeof(drp_filter), '
                   'sizeof(drp_change_src)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [C.sizeof(drp_amd.Splice), C.sizeof(drp_amd.Filter), C.sizeof(drp_amd.ChangeSrc)]
    assert C.sizeof(drp_amd.Splice) == 32
