"""GPU: the two emit kernels (drp_decode_spec.hip). emit_tiles<true> decodes Change payloads in
decode_change_fast's shapes (one-byte field tags, varints of 1..5 bytes) and lists any tile with
another shape; emit_tiles<false> re-emits those tiles with the general decoder. Streams here mix
both shapes inside the same tiles (and dense tiles past the 512-frame list), so every tile kind
goes through one of the two paths; results must equal the oracle's (protocol-buffers@2 decoding
as restated in oracle/; the oracle's decode of these shapes is held against an
independent model in tests/test_change_matrix.py, whose matrix the odd payloads also draw from)."""
import functools
import random

import pytest

import _change_model as M
import _oracle as O
import _streams as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from _gpu import drp_amd
    c = drp_amd.Ctx(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _matrix(valid):
    """tests/_change_model.py's matrix: the well-formed entries, or the malformed ones."""
    return [e.payload for e in M.change_matrix() if (M.decode(e.payload)["err"] == 0) == valid]


def _odd_payload(rng, kinds=8, malformed=True):
    """A Change payload outside the fast shapes: wide varints, a two-byte (non-minimal) tag,
    non-minimal lengths, unknown fields of each wire type, a repeated field, a missing one, or
    (kind 7) an entry of the model's matrix. malformed=False: only payloads that decode, so the
    stream goes on behind them."""
    key = bytes(rng.choice(b"abcdefghij") for _ in range(rng.randint(1, 30)))
    kind = rng.randrange(kinds)
    if kind == 7:
        return rng.choice(_matrix(True) if not malformed or rng.random() < 0.9 else _matrix(False))
    if kind == 5 and not malformed:
        kind = 4
    if kind == 0:  # change/from/to past 2^35: 6..8-byte varints
        return S.change_payload(key, rng.randint(2**35, 2**53 - 1), rng.randint(0, 2**53 - 1), 7)
    if kind == 1:  # the key tag as a two-byte varint (0x92 0x00 = 0x12)
        p = S.change_payload(key, 1, 2, 3)
        return b"\x92\x00" + p[1:]
    if kind == 2:  # a non-minimal length varint for the key
        return b"\x12" + bytes([0x80 | len(key), 0x00]) + key + b"\x18\x01\x20\x02\x28\x03"
    if kind == 3:  # unknown fields (numbers 9..12) of wire types 0, 2, 5 and 1
        return (S.change_payload(key, 4, 5, 6) + b"\x48\x96\x01" + b"\x52\x03abc" + b"\x5d\x01\x02\x03\x04" +
                b"\x61" + bytes(8))
    if kind == 4:  # a repeated field (the last one wins)
        return S.change_payload(key, 1, 2, 3) + b"\x18\x09"
    if kind == 5:  # a required field missing: a payload error at this frame
        return b"\x12" + S.varint(len(key)) + key + b"\x18\x01\x20\x02"
    return S.change_payload(key, rng.randint(0, 2**32 - 1), 1, 2, value=rng.randbytes(rng.randint(0, 3000)))


def _mixed(seed, nframes, odd_p, small_p=0.0, malformed=True, count=False):
    """count=True: (wire, frames it delivers when no payload is malformed: all but the id-0 headers)."""
    rng = random.Random(seed)
    parts, delivered = [], nframes
    for i in range(nframes):
        r = rng.random()
        if r < odd_p:
            parts.append(S.frame(_odd_payload(rng, malformed=malformed)))
        elif r < odd_p + small_p:
            blob = rng.random() < 0.5
            parts.append(S.frame(b"", 2) if blob else S.varint(rng.randint(0, 5)) + b"\x00")
            delivered -= 0 if blob else 1  # (an id-0 header is no frame)
        else:
            key = b"%010d" % i
            parts.append(S.frame(S.change_payload(key, i % 100 + 1, i % 128, (i + 1) % 128, rng.randbytes(64))))
    return (b"".join(parts), delivered) if count else b"".join(parts)


@pytest.mark.parametrize("seed,odd_p,small_p", [(1, 0.002, 0.0), (2, 0.05, 0.0), (3, 0.5, 0.0), (4, 0.01, 0.6), (5, 0.01, 0.99)])
def test_fast_and_general_emit_mix(ctx, seed, odd_p, small_p):
    from _gpu import assert_same
    wire = _mixed(seed, 40000, odd_p, small_p)
    assert_same(ctx.decode_batch(wire), O.decode_batch(wire), f"mix {seed}/{odd_p}/{small_p}")


@pytest.mark.parametrize("seed,odd_p,small_p", [(6, 0.05, 0.0), (7, 0.5, 0.0), (8, 0.05, 0.6)])
def test_emit_mix_without_errors_runs_to_the_end(ctx, seed, odd_p, small_p):
    """The streams above end at their first malformed payload (a missing field is one odd kind in
    eight), after a few hundred frames at most for odd_p >= 0.05 and 14 for odd_p = 0.5. Here every
    odd payload decodes, so all 40000 frames, the matrix's well-formed entries among them, go
    through the emit kernels."""
    from _gpu import assert_same
    wire, delivered = _mixed(seed, 40000, odd_p, small_p, malformed=False, count=True)
    assert delivered == 40000 or small_p
    ref = O.decode_batch(wire)
    assert (ref["err_code"], ref["tail"], ref["nframes"]) == (0, 0, delivered)
    assert_same(ctx.decode_batch(wire), ref, f"valid mix {seed}/{odd_p}/{small_p}")
