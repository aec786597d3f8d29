"""GPU parity of claims_fast's halo nodes (drp_decode_spec.hip: one lane per 16-byte halo block
builds the halo's live masks, halo_live16) against the oracle, with and without the per-frame
records, on short streams whose frames sit where the halo's block lanes, their lookahead and the
list's capacity can go wrong; and the prediction quality on a 4M-frame C2 stream, which identical
claims leave exactly where it was."""
import os
import random

import numpy as np
import pytest

import _oracle as O
import _streams as S
from _claims import _C2, filler, header_frame, live_count, place, straddle_streams  # noqa: F401

pytestmark = pytest.mark.gpu

TILE, HALO, FCAP = 8192, 512, 512  # drp_spec.h / drp_decode_spec.hip (NT 128)
IMG = TILE + HALO


def make_ctx(records):
    from _gpu import drp_amd
    keep = os.environ.get("DRP_CREC")
    os.environ["DRP_CREC"] = "1" if records else "0"
    try:
        c = drp_amd.Ctx(0)
    finally:
        if keep is None:
            os.environ.pop("DRP_CREC", None)
        else:
            os.environ["DRP_CREC"] = keep
    c.set_blob_skip(0)  # (every batch staged whole: the claims kernels see all of it)
    return c


@pytest.fixture(scope="module", params=[1, 0], ids=["records", "norecords"])
def ctx(request):
    c = make_ctx(request.param)
    yield c
    c.close()


# stream construction (frames at chosen byte positions, valid frames in between): tests/_claims.py


def dense_stream(total_want, halo_share):
    """Three quiet tiles; tile 1 and its halo hold a blob of zero bytes (every zero followed by a
    zero is a live position) sized so that tile 1 lists exactly total_want positions, halo_share of
    them in the halo."""
    rng = random.Random(43)
    for z in range(total_want, 2, -1):
        start = 2 * TILE + halo_share - z  # the zero run ends halo_share bytes into tile 1's halo
        blob = S.frame(bytes(z), 2)
        w = place([(start - (len(blob) - z), blob)], rng, end=4 * TILE, quiet=True)
        if live_count(w, TILE, TILE + IMG - 16) == total_want:
            assert live_count(w, TILE, 2 * TILE) <= FCAP or halo_share == 0
            return w
    raise AssertionError("no zero run gives %d live positions" % total_want)


def check(ctx, wire, label):
    from _gpu import assert_same
    assert_same(ctx.decode_batch(wire), O.decode_batch(wire, chunk=65536), label)


def test_headers_straddle_the_tile_end_and_every_halo_block_edge(ctx):
    for i, w in enumerate(straddle_streams()):
        assert len(w) <= 41 * TILE
        check(ctx, w, "straddle%d" % i)


def test_frames_start_in_the_last_bytes_of_the_image(ctx):
    """A frame starts in each of the image's last 19 bytes (the last 16 are never listed, the three
    before them have their lookahead there)."""
    rng = random.Random(47)
    items = [((d + 1) * TILE + HALO - d, _C2[d].tobytes()) for d in range(1, 20)]
    check(ctx, place(items, rng, end=21 * TILE + 300), "image_end")


def test_halo_without_live_positions(ctx):
    rng = random.Random(53)
    items = [(t * TILE - 100, S.frame(S.change_payload(b"quiet%d" % t, 1, 2, 3, value=b"\x55" * 1000)))
             for t in range(1, 6)]
    w = place(items, rng, end=6 * TILE + 500)
    for t in range(1, 6):
        assert live_count(w, t * TILE, t * TILE + HALO) == 0
    check(ctx, w, "quiet_halo")


@pytest.mark.parametrize("total,halo_share", [(FCAP, 60), (FCAP + 1, 60), (FCAP + 40, 300), (FCAP, 0), (FCAP + 1, 0)])
def test_list_capacity_with_the_halo(ctx, total, halo_share):
    """Tile + halo at FCAP positions (listed) and past it (the dense path), the halo holding the
    excess; and the same counts with an empty halo."""
    check(ctx, dense_stream(total, halo_share), "dense%d_%d" % (total, halo_share))


def test_stream_ends_inside_a_halo(ctx):
    base = S.c2_stream(700, seed=9).tobytes() + S.random_stream(random.Random(9), 300)
    assert len(base) > 7 * TILE + HALO
    for r in (1, 2, 3, 15, 16, 17, 18, 19, 100, 255, 256, 496, 497, 511, 512):
        for t in (3, 7):
            check(ctx, base[:t * TILE + r], "end_in_halo%d_%d" % (t, r))


def test_two_framings_take_the_jump_form(ctx):
    check(ctx, S.shadow_stream(40, period=8192, change_every=3), "shadow")
    check(ctx, S.shadow_stream(12, period=8192, shadow_at=300, small=100), "shadow_halo")


# verify_relisted of the 4M-frame C2 decode below (seed 21): the tiles whose predicted claims the
# records-only check hands to verify_counts. Measured on commit 4ec527b (the parent of the change
# that moved the halo's masks to one lane per block) in the same GPU session as the new build;
# identical claims give an identical count.
PARENT_RELISTED = {True: 158, False: 158}


def test_c2_predictions_unchanged_on_device():
    import ctypes as C
    import sys
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    from _gpu import drp_amd
    dev = torch.device("cuda", 0)
    n = 4_000_000
    wire = bench.c2_on_device(n, seed=21, dev=dev)
    so = torch.tensor([0, wire.numel()], dtype=torch.int64, device=dev)
    got, relisted = [], {}
    for on in (True, False):
        c = make_ctx(on)
        try:
            outs = bench.alloc_outputs(n + 64, dev)
            res = torch.zeros(C.sizeof(drp_amd.StreamResult), dtype=torch.uint8, device=dev)
            c.decode_device(wire, so, None, outs, n + 64, res)
            torch.cuda.synchronize()
            t = c.timing()
            print("records", on, "spec_repairs", t.spec_repairs, "strict_reruns", t.strict_reruns,
                  "verify_relisted", t.verify_relisted)
            assert t.spec_repairs == 0 and t.strict_reruns == 0
            relisted[on] = t.verify_relisted
            got.append({k: v[:n].cpu().numpy() for k, v in outs.items()})
        finally:
            c.close()
    assert relisted == PARENT_RELISTED
    for k in got[0]:
        np.testing.assert_array_equal(got[0][k], got[1][k], err_msg=k)
    assert int(got[0]["type"].min()) == 1 and int(got[0]["change"][12345]) == (12345 % 100) + 1
