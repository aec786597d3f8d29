"""claims_fast's per-frame record decode (drp_decode_spec.hip crec_frame / crec_general) compiled
as host C++ from the kernel's own source text: the harness of tests/test_claims_records.py, shared
with the tests of the merge-site generator (tests/test_merge_site.py)."""
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "dat-replication-protocol_amd", "csrc", "drp_decode_spec.hip")

HARNESS = r"""
#include <cstdint>
#include <cstdio>
#include <cstring>
#define __device__
#define __forceinline__
#define __builtin_amdgcn_alignbit(a, b, s) ((uint32_t)((((uint64_t)(a) << 32) | (uint32_t)(b)) >> (s)))
constexpr uint32_t CR_WORDS = 6;
%s
int main(int argc, char **argv) {
  FILE *f = fopen(argv[1], "rb");
  fseek(f, 0, SEEK_END);
  long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  static uint8_t *buf = new uint8_t[n + 256]();
  if (fread(buf, 1, n, f) != (size_t)n) return 1;
  fclose(f);
  FILE *g = fopen(argv[2], "r");
  unsigned long long o, id, tb;
  while (fscanf(g, "%%llu %%llu %%llu", &o, &id, &tb) == 3) {
    const unsigned long long base = o & ~8191ull;  // (tile-relative offsets, as on the device)
    const uint32_t *w32 = reinterpret_cast<const uint32_t *>(buf + base);
    uint32_t w[CR_WORDS];
    const bool ok = crec_frame(w32, (uint32_t)(o - base), (uint32_t)(n - base), (uint32_t)id, tb != 0, w);
    printf("%%d %%llu %%u %%u %%u %%u %%u %%u\n", ok, base, w[0], w[1], w[2], w[3], w[4], w[5]);
  }
  return 0;
}
"""


def functions(src, names):
    out = []
    for nm in names:
        m = re.search(r"^__device__ __forceinline__ \w+ " + nm + r"\(.*?^}\n", src, re.S | re.M)
        assert m, nm
        out.append(m.group(0))
    return "\n".join(out)


@pytest.fixture(scope="module")
def decoder():
    code = HARNESS % functions(open(SRC).read(), ["crec_general", "crec_frame"])
    d = tempfile.mkdtemp()
    cpp, exe = os.path.join(d, "crec.cpp"), os.path.join(d, "crec")
    open(cpp, "w").write(code)
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, cpp], check=True)
    return exe, d


def run(decoder, wire, frames):
    exe, d = decoder
    wp, fp = os.path.join(d, "wire.bin"), os.path.join(d, "frames.txt")
    open(wp, "wb").write(wire + b"\0" * 64)
    with open(fp, "w") as f:
        for o, i, tb in frames:
            f.write(f"{o} {i} {tb}\n")
    out = subprocess.run([exe, wp, fp], capture_output=True, text=True, check=True).stdout.split("\n")
    return [list(map(int, ln.split())) for ln in out if ln]


def header_starts(r, wire):
    """Each row's header offset: its payload offset minus the id byte and the length varint."""
    out = []
    for i in range(r["nframes"]):
        po, pl = int(r["payload_off"][i]), int(r["payload_len"][i])
        for k in (1, 2, 3):
            o = po - 1 - k
            if o < 0:
                continue
            v = wire[o:o + k]
            if all(b >= 0x80 for b in v[:-1]) and v[-1] < 0x80:
                L = sum((b & 0x7F) << (7 * j) for j, b in enumerate(v))
                if L == pl + 1 or (r["type"][i] & 0x80):
                    out.append(o)
                    break
        else:
            out.append(None)  # (a length varint of 4+ bytes: never a claims_fast node)
    return out
