"""GPU: the host-batch staging paths of drp_api.hip at small sizes, against the oracle's whole-batch
decode. The piece loop's capacity fallback (stage_pieces gives up, stage_batch stages the batch
whole and regrows its columns to the exact count), and the chunked copy pipeline with its early
fetch at 1 MiB chunks (DRP_PIPE_CHUNK=1), which the 280-300 MB batches of test_gpu_pipe.py reach
only at full size."""
import random

import numpy as np
import pytest

import _oracle as O
import _streams as S

pytestmark = pytest.mark.gpu

MiB = 1 << 20
# mirrored from drp_api.hip: stage_cap's first guess, the piece sizes and the least batch for pieces
PIECE_MIN = 64 << 10
PIECES_MIN = 1 << 20


def first_cap(nbytes):
    """stage_cap on a fresh ctx: one row per 32 bytes, and 1024."""
    return int(nbytes * (1.0 / 32)) + 1024


def as_u64(o):
    """A staged fetch's f64 columns back as integers (exact below 2^53)."""
    return {k: v.astype(np.uint64) if isinstance(v, np.ndarray) and v.dtype == np.float64 else v
            for k, v in o.items()}


# ---- the pieces give up: the batch is staged whole --------------------------------------------

NFRAMES = 786_432
TWO_BYTE_FRAMES = b"\x01\x02" * NFRAMES  # 1.5 MiB of empty blobs


@pytest.fixture(scope="module")
def fallback_refs():
    head = random.Random(77).randbytes(100)
    wires = {0: TWO_BYTE_FRAMES, 100: head + TWO_BYTE_FRAMES}
    return {brem: (w, O.decode_batch(w, blob_remaining=brem)) for brem, w in wires.items()}


@pytest.mark.parametrize("brem", [0, 100], ids=["plain", "carried_blob"])
def test_pieces_give_up_batch_staged_whole(fallback_refs, brem):
    """A fresh ctx (AUTO blob skip) probes its first host batch of >= 1 MiB in pieces. The first
    64 KiB piece holds 32,768 two-byte frames and the doubled second one 65,536, past the row guess
    of 1.5 MiB / 32 + 1024 = 50,176: stage_pieces returns its retry, stage_batch stages the batch
    whole and regrows to the exact count. With 100 carried blob bytes in front (row 0 of type 0x42)
    the fallback also has to restore the incoming carry and the error triple. (The batch is not
    pipelined, so no row was fetched early before the retry: the early fetch's reset after rows
    were fetched is not reached here.)"""
    from _gpu import assert_same, drp_amd
    wire, ref = fallback_refs[brem]
    assert ref["nframes"] == NFRAMES + (1 if brem else 0) and ref["err_code"] == 0
    if brem:
        assert ref["type"][0] == 0x42
    # the inputs force the path: pieces are tried, the first fits, the second overflows the guess
    body = len(wire) - brem
    cap = first_cap(body)
    first, second = PIECE_MIN // 2, 2 * PIECE_MIN // 2  # frames of the first piece and of the doubled one
    assert body >= PIECES_MIN and cap == 50_176
    assert first <= cap < first + second <= NFRAMES
    for staged in (False, True):
        with drp_amd.Ctx(0) as ctx:  # (fresh: no density learned, so the guess is the first one)
            g = ctx.decode_staged(wire, blob_remaining=brem) if staged else ctx.decode_batch(wire, blob_remaining=brem)
            assert_same(g, ref, f"fallback brem={brem} staged={staged}")


# ---- a small pipeline with early fetch ----------------------------------------------------------

CONT = 300_000


@pytest.fixture(scope="module")
def pipe_case():
    """~6 MiB: a carried continuation, C2 runs, two 1.5 MiB blobs (1 MiB chunk edges fall inside
    their payloads), a few hundred mixed frames and a blob the batch end cuts."""
    rng = random.Random(91)
    c2 = lambda n, start: S.c2_stream(n, seed=9 + start, start=start).tobytes()
    blob = lambda n: S.frame(rng.randbytes(n), 2)
    wire = b"".join([rng.randbytes(CONT), c2(9000, 0), blob(3 * MiB // 2 + 11), c2(9000, 9000),
                     blob(3 * MiB // 2 - 7), S.random_stream(rng, 400), c2(9000, 18000),
                     S.varint(2 * MiB + 1) + b"\x02" + rng.randbytes(400_000)])
    ref = O.decode_batch(wire, blob_remaining=CONT, cap=40_000)
    assert ref["err_code"] == 0 and ref["tail"] == 3 and ref["blob_remaining"] > 0  # (cut blob: DRP_TAIL_BLOB)
    assert 27_000 < ref["nframes"] < 39_000 and ref["type"][0] == 0x42
    return wire, ref


@pytest.fixture
def pipe_ctx(monkeypatch):
    from _gpu import drp_amd
    monkeypatch.setenv("DRP_PIPE_CHUNK", "1")  # (MiB; read when the ctx opens)
    c = drp_amd.Ctx(0)
    c.set_blob_skip(drp_amd.BLOB_SKIP_OFF)  # (straight to the pipelined whole-batch staging)
    yield c
    c.close()


def test_small_pipeline_with_early_fetch(pipe_ctx, pipe_case):
    """A pinned 6 MiB batch in 1 MiB chunks (seven with the half and quarter chunks at the end, four
    pieces: a piece jumps the blob it ends in) through the copy pipeline: drp_decode_batch into host
    columns (the early-fetch worker copies the rows of the earlier pieces during the copy), then the
    staged forms, all against the oracle's whole-batch decode, row 0 and the carry included."""
    import torch
    from _gpu import assert_same
    wire, ref = pipe_case
    pipe_chunk = 1 * MiB
    assert len(wire) >= 2 * pipe_chunk and len(wire) - CONT >= 2 * pipe_chunk
    t = torch.empty(len(wire), dtype=torch.uint8, pin_memory=True)
    a = t.numpy()
    a[:] = np.frombuffer(wire, np.uint8)
    g = pipe_ctx.decode_batch(a, blob_remaining=CONT, cap=40_000)
    assert_same(g, ref, "pipe batch")
    assert pipe_ctx.timing().h2d_skipped == 0
    assert_same(pipe_ctx.decode_staged(a, blob_remaining=CONT, pieces=3), ref, "pipe staged")
    assert pipe_ctx.timing().h2d_skipped == 0
    assert_same(as_u64(pipe_ctx.decode_staged(a, blob_remaining=CONT, block=True, f64=True)), ref, "pipe block f64")
    del t
