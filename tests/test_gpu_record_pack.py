"""GPU parity of the stored form of claims_fast's per-frame records (crec_pack in fast_records,
crec_unpack in emit_recs, drp_decode_spec.hip) against the oracle: narrow records (change, from and
to all below the limit: 3 words) and wide ones (5 words) mixed per frame, per half wave and per
run of tiles; streams of one frame, one tile and three tiles; blobs and value-less Changes among
narrow ones with a subset frame's tile left to the wire-reading emission; and one context decoding
wide, then narrow, then mixed records over the same slots, so that a narrow record's unwritten
wide words hold the wide batch's numbers. The words themselves: tests/test_record_pack.py."""
import os
import random
import re

import pytest

import _oracle as O
import _streams as S
from test_gpu_records import rec_ctx

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "dat-replication-protocol_amd", "csrc", "drp_decode_spec.hip")
LIMIT = 1 << int(re.search(r"CRP_NB = (\d+)", open(SRC).read()).group(1))

NARROW = [LIMIT - 1, 0, 1, 127, 128, LIMIT // 2]
WIDE = [LIMIT, 2 ** 32 - 1, LIMIT + 1, 70000, 2 ** 31]


@pytest.fixture(scope="module")
def ctx():
    c = rec_ctx()
    c.set_blob_skip(0)
    yield c
    c.close()


def c2_like(i, wide, rng, value=True):
    """A C2-shaped frame (10-digit key, 64 value bytes); wide: one of the three numbers (in turn) at
    or above the limit, the others narrow."""
    nums = [NARROW[(i + j) % len(NARROW)] for j in range(3)]
    if wide:
        nums[i % 3] = WIDE[(i // 3) % len(WIDE)]
    return S.frame(S.change_payload(b"%010d" % i, *nums, value=rng.randbytes(64) if value else None))


def check(ctx, wire, label):
    from _gpu import assert_same
    assert_same(ctx.decode_batch(wire), O.decode_batch(wire, chunk=65536), label)


@pytest.mark.parametrize("period", [1, 32, 200])
def test_narrow_and_wide_mixed(ctx, period):
    """~20,000 frames switching between narrow and wide every `period` frames: lanes of one wave
    (1), half waves (32), and whole narrow tiles, whole wide tiles and mixed ones (200: a tile
    holds ~95 frames)."""
    rng = random.Random(period)
    wire = b"".join(c2_like(i, (i // period) & 1, rng) for i in range(20_000))
    check(ctx, wire, f"period{period}")


@pytest.mark.parametrize("n", [1, 96, 200])
def test_small_streams(ctx, n):
    """One frame, one tile, three tiles (every third frame wide)."""
    rng = random.Random(n)
    wire = b"".join(c2_like(i, i % 3 == 1, rng) for i in range(n))
    check(ctx, wire, f"n{n}")


def test_blobs_valueless_and_a_subset(ctx):
    """Narrow Changes among small blobs (2 words) and Changes without a value, and one frame with
    a subset in the middle: its tile takes the wire-reading emission, the tiles around it their
    records."""
    rng = random.Random(7)
    parts = []
    for i in range(6000):
        if i % 7 == 3:
            parts.append(S.frame(rng.randbytes(rng.randrange(0, 40)), 2))
        parts.append(c2_like(i, False, rng, value=i % 5 != 2))
        if i == 3000:
            parts.append(S.frame(S.change_payload(b"with-subset", 1, 2, 3, value=b"v" * 20, subset=b"sub")))
    check(ctx, b"".join(parts), "blobs")


def test_stale_wide_words():
    """Wide, then narrow, then mixed records on one context, every frame of the same size in all
    three (numbers of two bytes: 128 .. limit - 1 narrow, limit .. 16383 wide), so each record
    lands in the slot the batch before wrote: the narrow records' wide words keep the wide batch's
    numbers, and only a record's own first word may say whether they are read."""
    rng = random.Random(11)

    def stream(kind):
        out = []
        for i in range(20_000):
            wide = kind == "wide" or (kind == "mixed" and rng.randrange(2))
            nums = [rng.randrange(LIMIT, 16384) if wide else rng.randrange(128, LIMIT) for _ in range(3)]
            if wide and kind == "mixed":
                nums[rng.randrange(3)] = rng.randrange(128, LIMIT)  # (wide by two of its numbers only)
            out.append(S.frame(S.change_payload(b"%010d" % i, *nums, value=rng.randbytes(64))))
        return b"".join(out)

    wires = {k: stream(k) for k in ("wide", "narrow", "mixed")}
    assert len(set(map(len, wires.values()))) == 1
    c = rec_ctx()
    try:
        c.set_blob_skip(0)
        for k in ("wide", "narrow", "mixed"):
            check(c, wires[k], k)
    finally:
        c.close()
