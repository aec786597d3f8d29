"""CPU check of claims_fast's per-block halo live masks (drp_decode_spec.hip halo_live16, compiled
here as host C++ from the kernel's own source text): one 16-byte block per lane, with the next
block's low bits as lookahead, marks exactly the positions the 64-position form of the tile's
threads marks (restated below as it stood when eight lanes built the halo's masks), and both mark
exactly the starts of a 1..3-byte varint followed by an id <= 2."""
import os
import re
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "dat-replication-protocol_amd", "csrc", "drp_decode_spec.hip")
HALO = 528  # 33 blocks of 16 bytes: the halo's 32 and the lookahead of the last
NB = HALO // 16

HARNESS = r"""
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#define __host__
#define __device__
#define __forceinline__
%s
// masks16's contract: bit k = MSB of byte k (m), bit 16 + k = byte k <= 2 (s)
static uint32_t masks16_ref(const uint8_t *b) {
  uint32_t w = 0;
  for (int k = 0; k < 16; k++) w |= (uint32_t)(b[k] >> 7) << k | (uint32_t)(b[k] <= 2) << (16 + k);
  return w;
}
// the 64-position form (one lane per 64 bytes: four blocks and the next one's masks)
static uint64_t live64(const uint32_t *hk) {
  const uint64_t hM0 = (uint64_t)(hk[0] & 0xFFFFu) | ((uint64_t)(hk[1] & 0xFFFFu) << 16) |
                       ((uint64_t)(hk[2] & 0xFFFFu) << 32) | ((uint64_t)(hk[3] & 0xFFFFu) << 48);
  const uint64_t hS0 = (uint64_t)(hk[0] >> 16) | ((uint64_t)(hk[1] >> 16) << 16) | ((uint64_t)(hk[2] >> 16) << 32) |
                       ((uint64_t)(hk[3] >> 16) << 48);
  const uint64_t hM1 = hk[4] & 0xFFFFu, hS1 = hk[4] >> 16;
  const uint64_t hX0 = ~hM0 & ((hS0 >> 1) | (hS1 << 63)), hX1 = ~hM1 & (hS1 >> 1);
  const uint64_t hXs1 = (hX0 >> 1) | (hX1 << 63), hXs2 = (hX0 >> 2) | (hX1 << 62), hMs1 = (hM0 >> 1) | (hM1 << 63);
  return hX0 | (hM0 & (hXs1 | (hMs1 & hXs2)));
}
int main(int argc, char **argv) {
  constexpr int NB = 33, HB = 32;
  FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
  if (!f || !o) return 1;
  const int past = argv[3][0] == '1';  // the kernel's word past the image: no terminators
  uint8_t h[NB * 16];
  while (fread(h, 1, sizeof h, f) == sizeof h) {
    uint32_t w[NB];
    for (int j = 0; j < NB; j++) w[j] = masks16_ref(h + 16 * j);
    if (past) w[HB] = 0xFFFFu;
    uint16_t out[2 * HB];
    for (int s = 0; s < HB / 4; s++) {
      const uint64_t l = live64(w + 4 * s);
      for (int k = 0; k < 4; k++) out[4 * s + k] = (uint16_t)(l >> (16 * k));
    }
    for (int j = 0; j < HB; j++) {
      const uint32_t l = halo_live16(w[j], w[j + 1]);
      if (l >> 16) return 2;  // (positions 0..15 only)
      out[HB + j] = (uint16_t)l;
    }
    fwrite(out, 2, 2 * HB, o);
  }
  fclose(o);
  return 0;
}
"""


def helper_source():
    src = open(SRC).read()
    m = re.search(r"^__host__ __device__ __forceinline__ uint32_t halo_live16\(.*?^}\n", src, re.S | re.M)
    assert m, "halo_live16"
    return m.group(0)


def run_harness(halos, past):
    """(64-position masks, per-block masks) of every halo, each [n, 32] uint16."""
    assert halos.dtype == np.uint8 and halos.shape[1] == HALO
    d = tempfile.mkdtemp()
    cpp, exe = os.path.join(d, "h.cpp"), os.path.join(d, "h")
    inp, out = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    open(cpp, "w").write(HARNESS % helper_source())
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, cpp], check=True)
    halos.tofile(inp)
    subprocess.run([exe, inp, out, "1" if past else "0"], check=True)
    r = np.fromfile(out, np.uint16).reshape(len(halos), 64)
    return r[:, :32], r[:, 32:]


def live_by_definition(h):
    """Bit p of block j: a varint of 1..3 bytes starts at 16 j + p and a byte <= 2 follows it."""
    h = h.astype(np.int64)
    n = h.shape[1]
    msb, le2 = h >= 0x80, h <= 2
    pad = lambda a, k: np.pad(a[:, k:], ((0, 0), (0, k)))  # noqa: E731  (a[p + k], false past the end)
    x = ~msb & pad(le2, 1)
    live = x | (msb & pad(x, 1)) | (msb & pad(msb, 1) & pad(x, 2))
    bits = live[:, :512].reshape(len(h), 32, 16)
    assert n == HALO
    return (bits * (1 << np.arange(16))).sum(axis=2).astype(np.uint16)


def adversarial():
    out = []
    for fill in (0x80, 0xFF, 0x00, 0x01, 0x02, 0x7F):
        out.append(np.full(HALO, fill, np.uint8))
    # alternating continuation / small bytes: every position a candidate of some length
    for pat in ([0x80, 0x00], [0x80, 0x80, 0x01], [0x80, 0x80, 0x80, 0x02], [0x05, 0x01], [0x00, 0x80, 0x02]):
        for sh in range(len(pat)):
            out.append(np.resize(np.roll(np.array(pat, np.uint8), sh), HALO))
    # 1-, 2- and 3-byte varints ending at every offset around each 16-byte (and so 64-byte) edge,
    # and at every offset of the last 16 bytes and the lookahead block
    ends = sorted({b + d for b in range(16, HALO, 16) for d in range(-4, 5)} | set(range(490, HALO - 1)))
    for bg in (0x55, 0xFF):
        for e in ends:
            for k in (1, 2, 3):
                for idb in (0, 1, 2, 3):
                    if e - k + 1 < 0 or e + 1 >= HALO:
                        continue
                    h = np.full(HALO, bg, np.uint8)
                    h[e - k + 1:e] = 0x80
                    h[e] = 0x05
                    h[e + 1] = idb
                    out.append(h)
    return np.stack(out)


def test_block_masks_match_the_64_position_form_on_random_halos():
    rng = np.random.default_rng(17)
    n = 100_000
    uniform = rng.integers(0, 256, size=(n, HALO), dtype=np.uint8)
    # biased: continuation bytes, ids and small lengths dominate (most positions are candidates)
    alphabet = np.array([0, 1, 2, 2, 0x80, 0x80, 0x85, 0xFF, 0x03, 0x55], np.uint8)
    biased = alphabet[rng.integers(0, len(alphabet), size=(n, HALO))]
    halos = np.concatenate([uniform, biased])
    for past in (False, True):
        ref, new = run_harness(halos, past)
        assert ref.any() and np.array_equal(ref, new), past
    ref, new = run_harness(halos[::50], False)
    np.testing.assert_array_equal(new, live_by_definition(halos[::50]))


def test_block_masks_on_adversarial_halos():
    halos = adversarial()
    want = live_by_definition(halos)
    for past in (False, True):
        ref, new = run_harness(halos, past)
        bad = np.argwhere(ref != new)
        assert len(bad) == 0, (past, bad[:4])
        if not past:
            np.testing.assert_array_equal(new, want)
        else:  # only the last block's positions 13..15 see the word past the image
            np.testing.assert_array_equal(new[:, :31], want[:, :31])
            np.testing.assert_array_equal(new[:, 31] & 0x1FFF, want[:, 31] & 0x1FFF)
