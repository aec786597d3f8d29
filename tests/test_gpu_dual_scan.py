"""GPU parity of the tail's two-array tile scan (scan_reduce2 / scan_top2 / scan_down2,
drp_decode_spec.hip) against the oracle: device decodes of 3 streams of C2 frames with a small
blob after every 6th, so that a stream's changes differ from its frames and both running sums
matter. A scan block covers 4096 tiles. The largest case has ~4200 tiles: one stream ends in block
0, one crosses tile 4096 and one lies wholly in block 1, so the second block's offsets of both
sums (scan_top2's second array, bsum[gridDim.x + blockIdx.x]) reach the streams' results. The
launcher picks its form by its bound on the tile count (bytes / 8192 + 2 * streams + 2): the next
two cases sit on either side of it (4097: reduce, top and down; 4096: the one-block launch); the
smallest decodes are three streams sharing two tiles, and one stream of one tile. (Capacity
overflow: tests/test_gpu_change_matrix.py.)"""
import functools

import numpy as np
import pytest

import _streams as S
from _tail import device_decode_check, stream_refs, tail_ctx

pytestmark = pytest.mark.gpu

TILE = 8192
BLOCK = 4096  # tiles per scan block (SCAN_SPAN)
BLOB = np.frombuffer(S.frame(b"small blob payload", 2), np.uint8)
GROUP = 6 * 86 + len(BLOB)  # six C2 frames and the blob
MAX_BYTES = 4200 * TILE + 100


@functools.lru_cache(maxsize=None)
def groups(n):
    c2 = S.c2_stream(6 * n, seed=13).reshape(n, 6 * 86)
    return np.concatenate([c2, np.broadcast_to(BLOB, (n, len(BLOB)))], axis=1).reshape(-1)


def tile_prefix(cuts):
    """The decode's tiles per stream (every tile a stream touches), as a running sum."""
    n = [(b + TILE - 1) // TILE - a // TILE for a, b in zip(cuts[:-1], cuts[1:])]
    return [0] + [int(x) for x in np.cumsum(n)]


def near_tile(t):
    """The group boundary at or before tile t's first byte."""
    return t * TILE // GROUP * GROUP


@functools.lru_cache(maxsize=None)
def case(nbytes, inner):
    """Streams over the first nbytes of the grouped wire, cut at the group boundaries `inner`
    (entry 0), the last one ending wherever nbytes does (a cut frame is its tail)."""
    wire = groups(MAX_BYTES // GROUP + 1)[:nbytes].tobytes()
    cuts = [0, *inner, nbytes]
    entry = [0] * (len(cuts) - 1)
    refs = stream_refs(wire, cuts, entry)
    return wire, cuts, entry, refs, sum(r["nframes"] for r in refs)


# name: bytes, the streams' inner cuts
SIZES = {"two_blocks": (MAX_BYTES, (near_tile(4000), near_tile(4130))),
         "bound_4097": (4089 * TILE + 100, (near_tile(1363), near_tile(2726))),
         "bound_4096": (4088 * TILE + 100, (near_tile(1363), near_tile(2726))),
         "three_in_two_tiles": (21 * GROUP + 50, (7 * GROUP, 14 * GROUP)),
         "one_tile": (5000, ())}
BOUND = {"bound_4097": 4097, "bound_4096": 4096}  # the launcher's tile bound at those sizes


@pytest.fixture(scope="module")
def ctx():
    c = tail_ctx(1)
    yield c
    c.close()


@pytest.mark.parametrize("size", list(SIZES))
def test_rows_and_stream_counts(ctx, size):
    nbytes, inner = SIZES[size]
    args = case(nbytes, inner)
    cuts = args[1]
    ns = len(cuts) - 1
    tp = tile_prefix(cuts)
    if size in BOUND:
        assert nbytes // TILE + 2 * ns + 2 == BOUND[size]
    if size == "two_blocks":
        # real tiles: stream 0 in block 0, stream 1 across the block edge, stream 2 in block 1
        assert tp[1] < BLOCK < tp[2] and tp[3] >= 4200, tp
        ch = [int(((r["type"][:r["nframes"]] & 0x3F) == 1).sum()) for r in args[3]]
        assert all(0 < c < r["nframes"] for c, r in zip(ch, args[3])), ch  # changes != frames
    if size == "three_in_two_tiles":  # (tiles are aligned to the wire: streams share them)
        assert tp == [0, 1, 2, 4], tp
    if size == "one_tile":
        assert tp == [0, 1], tp
    device_decode_check(ctx, *args)
