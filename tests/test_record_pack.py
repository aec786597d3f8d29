"""CPU check of the stored form of claims_fast's per-frame records (drp_decode_spec.hip crec_pack /
crec_unpack, compiled here as host C++ from the kernel's own source text, with crec_frame /
crec_general in front of them as fast_records has them): crec_unpack gives back exactly the
words crec_pack was given, for every record crec_frame accepts and over every field's declared
range; the narrow flag is set exactly when change, from and to are all below the limit; a record
takes 2 (blob), 3 (narrow Change) or 5 (wide Change) words, and crec_unpack reads no word past
them (the harness poisons those before it unpacks: on the device they hold an earlier batch's
bytes); a field past its width is refused, never truncated. The GPU side is
tests/test_gpu_record_pack.py."""
import os
import random
import re
import subprocess
import tempfile

import pytest

import _streams as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "dat-replication-protocol_amd", "csrc", "drp_decode_spec.hip")
TEXT = open(SRC).read()
CONSTS = re.search(r"^constexpr uint32_t CR_PWORDS = .*$", TEXT, re.M).group(0)
K = {k: int(v) for k, v in re.findall(r"(\w+) = (\d+)[,;]", CONSTS)}
LIMIT = 1 << K["CRP_NB"]
NARROW_BIT = 25  # (the layout comment above CR_CAP)

HARNESS = r"""
#include <cstdint>
#include <cstdio>
#include <cstring>
#define __device__
#define __forceinline__
#define __builtin_amdgcn_alignbit(a, b, s) ((uint32_t)((((uint64_t)(a) << 32) | (uint32_t)(b)) >> (s)))
constexpr uint32_t CR_WORDS = 6;
%s
%s
// pack, poison the words the record does not hold, unpack: "ok np narrow same w0..w5"
static void round_trip(bool ok, const uint32_t (&w)[CR_WORDS]) {
  uint32_t p[CR_PWORDS], u[CR_WORDS];
  const uint32_t np = crec_pack(w, p);
  for (uint32_t k = np; k < CR_PWORDS && np; k++) p[k] = 0xDEADBEEFu ^ (k * 0x01010101u);
  for (uint32_t k = 0; k < CR_WORDS; k++) u[k] = 0xA5A5A5A5u;
  if (np) crec_unpack(p, u);
  printf("%%d %%u %%u %%d %%u %%u %%u %%u %%u %%u\n", ok, np, (p[0] >> %d) & 1u, np && !memcmp(u, w, sizeof(u)), w[0], w[1],
         w[2], w[3], w[4], w[5]);
}
int main(int argc, char **argv) {
  FILE *f = fopen(argv[1], "rb");
  fseek(f, 0, SEEK_END);
  long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  static uint8_t *buf = new uint8_t[n + 256]();
  if (fread(buf, 1, n, f) != (size_t)n) return 1;
  fclose(f);
  FILE *g = fopen(argv[2], "r");
  char mode;
  unsigned long long a[6];
  while (fscanf(g, " %%c", &mode) == 1) {
    uint32_t w[CR_WORDS];
    if (mode == 'F') {  // a frame of the wire: header offset, id, cut blob
      if (fscanf(g, "%%llu %%llu %%llu", &a[0], &a[1], &a[2]) != 3) return 2;
      const unsigned long long base = a[0] & ~8191ull;  // (tile-relative offsets, as on the device)
      const bool ok = crec_frame(reinterpret_cast<const uint32_t *>(buf + base), (uint32_t)(a[0] - base),
                                 (uint32_t)(n - base), (uint32_t)a[1], a[2] != 0, w);
      round_trip(ok, w);
    } else {  // six record words as they are
      if (fscanf(g, "%%llu %%llu %%llu %%llu %%llu %%llu", &a[0], &a[1], &a[2], &a[3], &a[4], &a[5]) != 6) return 2;
      for (int k = 0; k < 6; k++) w[k] = (uint32_t)a[k];
      round_trip(true, w);
    }
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
def packer():
    code = HARNESS % (CONSTS, functions(TEXT, ["crec_general", "crec_frame", "crec_pack", "crec_unpack"]), NARROW_BIT)
    d = tempfile.mkdtemp()
    cpp, exe = os.path.join(d, "crp.cpp"), os.path.join(d, "crp")
    open(cpp, "w").write(code)
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, cpp], check=True)
    return exe, d


def run(packer, wire, lines):
    exe, d = packer
    wp, fp = os.path.join(d, "wire.bin"), os.path.join(d, "in.txt")
    open(wp, "wb").write(wire + b"\0" * 64)
    open(fp, "w").write("\n".join(lines) + "\n")
    out = subprocess.run([exe, wp, fp], capture_output=True, text=True, check=True).stdout.split("\n")
    got = [list(map(int, ln.split())) for ln in out if ln]
    assert len(got) == len(lines)
    return got


def check(rows, want_ok=None):
    """Every accepted record: round trip exact, size by kind, narrow flag by the numbers."""
    n = 0
    for j, (ok, np_, narrow, same, w0, pl, w2, n0, n1, n2) in enumerate(rows):
        if want_ok is not None:
            assert ok == want_ok[j], (j, ok)
        if not ok:
            continue
        n += 1
        change = (w0 >> 14) & 3 == 1
        small = max(n0, n1, n2) < LIMIT
        assert same == 1, (j, np_, w0, pl, w2, n0, n1, n2)
        assert np_ == (2 if not change else 3 if small else 5), (j, np_)
        assert narrow == (1 if small else 0), (j, narrow, n0, n1, n2)
    return n


def frames_of(payloads, typ=1):
    wire, lines = b"", []
    for p in payloads:
        lines.append(f"F {len(wire)} {typ} 0")
        wire += S.frame(p, typ)
    return wire, lines


def test_c2_stream(packer):
    wire = S.c2_stream(5000).tobytes()
    rows = run(packer, wire, [f"F {86 * i} 1 0" for i in range(5000)])
    # (the last frames' field headers are less than 36 bytes before the end: not recorded)
    assert check(rows) >= 4999 and all(r[1] == 3 for r in rows if r[0])


def test_wide_stream(packer):
    rng = random.Random(5)
    wire, lines = frames_of([S.change_payload(b"key%07d" % i, 1000 + i * 37, i * 7919, 2 ** 31 + i,
                                              value=bytes(rng.randrange(256) for _ in range(40))) for i in range(3000)])
    rows = run(packer, wire, lines)
    assert check(rows, [1] * 3000) == 3000 and all(r[1] == 5 for r in rows)


def test_numbers_around_the_limit(packer):
    vals = [0, LIMIT - 1, LIMIT, 2 ** 32 - 1]
    combos = [(a, b, c) for a in vals for b in vals for c in vals]
    assert len(combos) == 64
    for value in (None, b"v" * 9):
        wire, lines = frames_of([S.change_payload(b"k%d" % i, a, b, c, value=value) for i, (a, b, c) in enumerate(combos)])
        rows = run(packer, wire + b"\0" * 64, lines)
        assert check(rows, [1] * 64) == 64
        for (a, b, c), r in zip(combos, rows):
            assert r[7:] == [a, b, c] and r[1] == (3 if max(a, b, c) < LIMIT else 5)


def test_key_and_value_lengths(packer):
    cases = [(kl, vl, wide) for kl in (1, 127, 128, 16383) for vl in (None, 0, 1, 127, 128, 20000) for wide in (0, 1)]
    pays = [S.change_payload(b"k" * kl, 1, LIMIT if wide else 2, 3, value=None if vl is None else b"v" * vl)
            for kl, vl, wide in cases]
    wire, lines = frames_of(pays)
    rows = run(packer, wire + b"\0" * 64, lines)
    # (crec_frame's one-byte-number form takes a value length of <= 2 bytes: the 20000-byte value
    # is recorded behind numbers of two bytes or more, its general form)
    want = [0 if vl == 20000 and not wide else 1 for kl, vl, wide in cases]
    assert check(rows, want) == sum(want) == len(pays) - 4
    for p, r in zip(pays, rows):
        assert r[5] == len(p)


def test_blobs(packer):
    wire, lines = frames_of([b"", b"x", b"y" * 127, b"z" * 128, b"b" * 70000, b"c" * (2 ** 21 - 2)], typ=2)
    lines.append(f"F {len(wire)} 2 1")
    wire += S.frame(b"x" * 300, 2)[:100]  # (cut by the stream end: delivered, PARTIAL)
    rows = run(packer, wire, lines)
    assert check(rows, [1] * 7) == 7 and all(r[1] == 2 for r in rows)
    assert rows[-1][5] == 300 and (rows[-1][4] >> 16) & 1 == 1 and rows[-2][5] == 2 ** 21 - 2


def words(po, ident, partial, hv, kb, vd, pl, klen, nums):
    if ident != 1:
        return [po | ident << 14 | partial << 16, pl, 0, 0, 0, 0]
    vo = 1 + kb + klen + vd if hv else 0
    return [po | 1 << 14 | partial << 16 | hv << 17 | kb << 18, pl, klen | vo << 16, *nums]


def test_random_field_tuples(packer):
    """100k records drawn over each field's whole width (payload offset 14 bits, payload length
    CRP_PL_BITS, key length CRP_KL_BITS, value offset past the key CRP_VD_BITS, numbers 32), each
    field at its maximum or zero in about a tenth of the draws."""
    rng = random.Random(2024)

    def draw(bits):
        x = rng.random()
        return (1 << bits) - 1 if x < 0.1 else 0 if x < 0.15 else rng.randrange(1 << bits)

    lines, kinds = [], set()
    for _ in range(100_000):
        ident, hv = rng.choice([1, 1, 1, 2]), rng.randrange(2)
        narrow = rng.randrange(2)
        nums = [draw(K["CRP_NB"]) if narrow else draw(32) for _ in range(3)]
        w = words(draw(14), ident, rng.randrange(2), hv, rng.choice([1, 2]), draw(K["CRP_VD_BITS"]) if hv else 0,
                  draw(K["CRP_PL_BITS"]), draw(K["CRP_KL_BITS"]), nums)
        kinds.add((ident, hv, max(nums) < LIMIT))
        lines.append("W " + " ".join(map(str, w)))
    top = words(2 ** 14 - 1, 1, 1, 1, 2, 2 ** K["CRP_VD_BITS"] - 1, 2 ** K["CRP_PL_BITS"] - 1, 2 ** K["CRP_KL_BITS"] - 1,
                [2 ** 32 - 1] * 3)
    lines.append("W " + " ".join(map(str, top)))  # (every field at its maximum at once)
    assert len(kinds) == 8
    rows = run(packer, b"", lines)
    assert check(rows) == len(lines)


def test_fields_past_their_width_are_refused(packer):
    """crec_pack never truncates: a field one past its width gives 0 words (fast_records then
    leaves the tile without records)."""
    fit = dict(po=100, ident=1, partial=0, hv=1, kb=1, vd=8, pl=500, klen=10, nums=[1, 2, 3])
    over = [dict(fit, pl=2 ** K["CRP_PL_BITS"]), dict(fit, pl=2 ** 32 - 1), dict(fit, klen=2 ** K["CRP_KL_BITS"]),
            dict(fit, vd=2 ** K["CRP_VD_BITS"]), dict(fit, ident=2, pl=2 ** K["CRP_PL_BITS"])]
    lines = ["W " + " ".join(map(str, words(**f))) for f in [fit] + over]
    w = words(**fit)
    lines.append("W " + " ".join(map(str, [w[0], w[1], w[2] & 0xFFFF | 5 << 16, *w[3:]])))  # (value before the key's end)
    lines.append("W " + " ".join(map(str, [w[0] | 1 << 20, *w[1:]])))  # (a bit above w0's fields)
    rows = run(packer, b"", lines)
    assert [r[1] for r in rows] == [3] + [0] * (len(lines) - 1)
