"""GPU parity of the speculative decode's tail (drp_launch_spec_tail, drp_decode_spec.hip) against
the oracle: one scan gives the row bases and the change-count bases before emission, zeroes the
deferred-tile count and marks emit_recs' chunks; emit_sparse, emit_recs, emit_lean, emit_tiles and
stream_counts then run behind it on the decode stream. Every case runs with claims_fast's records
on and off (DRP_CREC), so that the emitters beside emit_recs own rows in every batch (records off:
every tile's; records on: the tiles that refuse records)."""
import functools
import random

import pytest

import _oracle as O
import _streams as S
from _tail import cut_entries, device_decode_check, stream_refs, tail_ctx

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module", params=(1, 0), ids=("rec1", "rec0"))
def ctx(request):
    c = tail_ctx(request.param)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def mixed_wire(seed=3):
    """~20k frames in which every emitter owns rows: C2-shaped tiles (emit_recs), a Change with a
    subset (its tile refuses records), ~600 value-less Changes of 14 bytes (more than 128 frames
    per tile), 40 C5-shaped frames (two per tile: the sparse form) and two 40 KB blobs (runs of
    empty tiles: emit_recs' search form)."""
    rng = random.Random(seed)
    c2 = lambda n, start: S.c2_stream(n, seed=seed + start, start=start).tobytes()
    parts = [c2(4000, 0),
             S.frame(S.change_payload(b"with-subset", 1, 2, 3, value=b"v" * 20, subset=b"sub")),
             c2(4000, 4000),
             b"".join(S.frame(S.change_payload(b"%04d" % i, i % 100, 2, 3)) for i in range(600)),
             c2(4000, 8000),
             S.c5_stream(rng, 40),
             c2(3000, 12000),
             S.frame(rng.randbytes(40_000), 2),
             c2(2500, 15000),
             S.frame(rng.randbytes(40_000), 2),
             c2(2000, 17500)]
    return b"".join(parts)


@functools.lru_cache(maxsize=None)
def other_wire():
    """A batch of another tile count than mixed_wire's (the stale-state case's Y)."""
    rng = random.Random(19)
    return S.c2_stream(3001, seed=5).tobytes() + S.random_stream(rng, 700) + S.c5_stream(rng, 9)


@functools.lru_cache(maxsize=None)
def shadow_wire():
    return S.shadow_stream(300, period=8192, change_every=3)


@functools.lru_cache(maxsize=None)
def oracle(wire_fn):
    return O.decode_batch(wire_fn(), chunk=65536)


def check(ctx, wire_fn, label):
    from _gpu import assert_same
    assert_same(ctx.decode_batch(wire_fn()), oracle(wire_fn), label)


def test_mixed_batch(ctx):
    check(ctx, mixed_wire, "mixed")


def test_failed_prediction(ctx):
    """Two framings that never merge: the first tail does nothing (the emitters see the miss flag),
    repair passes clear and refill the lists, and the tail runs a second time."""
    check(ctx, shadow_wire, "shadow")
    assert ctx.timing().spec_repairs > 0


def test_stale_scan_sums_chunk_marks_and_deferred_list(ctx):
    """X, Y, X on one context, X and Y of different tile counts: the scan's block sums, the chunk
    marks and the deferred-tile list are all left over from the decode before."""
    assert len(mixed_wire()) // 8192 != len(other_wire()) // 8192
    for k, fn in enumerate([mixed_wire, other_wire, mixed_wire]):
        check(ctx, fn, f"stale{k}")


# ---- device decode of many streams (helpers: tests/_tail.py) ----------------------------------

@functools.lru_cache(maxsize=None)
def cut_case():
    rng = random.Random(505)
    wire = S.random_stream(rng, 30_000, blob_p=0.02, blob_max=30000) + S.c2_stream(20_000, seed=8).tobytes()
    cuts = sorted(set([0] + rng.sample(range(1, len(wire)), 149) + [len(wire)]))
    entry, nrows = cut_entries(wire, cuts)
    return wire, cuts, entry, stream_refs(wire, cuts, entry), nrows


def test_device_decode_of_many_streams(ctx):
    """~150 streams cut at arbitrary bytes: stream_counts reads the change-count bases that the scan
    wrote before emission."""
    device_decode_check(ctx, *cut_case())
