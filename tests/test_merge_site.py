"""CPU checks of tests/_streams.merge_site, the generator behind tests/test_gpu_record_repair.py:
a host frame whose payload holds a chain of well-formed frames that ends exactly where the host
does, so that a decode started on the chain merges with the real framing at the first frame after
the host (decode.js:144-262 has one framing; the second one exists only for a decoder that
predicts entries). The GPU tests rely on the geometry asserted here: the real entry of tile t lies
in segment k, tile t - 1 holds host payload only, the chain's frames precede the entry inside
tile t, and every frame of tile t is in the shape claims_fast records (crec_frame, compiled from the
kernel's own source by tests/_crec.py), at most CR_CAP = 128 of them."""
import numpy as np
import pytest

import _oracle as O
import _streams as S
from _crec import decoder, run  # noqa: F401  (decoder: the compiled harness, a fixture)

KS = [1, 2, 63, 64, 65, 127]
PRE, POST, SLEN = 150, 200, 100
CR_CAP = 128
COLS = O.COLS32 + O.COLS64 + ["flags"]
ID = {"blob": 2, "narrow": 1, "wide": 1}


def tile_frames(wire, m, ref):
    """Tile t's frames as (header offset, id): the chain's before the host's end, the real ones after."""
    lo, hi = m["t"] * S.TILE, (m["t"] + 1) * S.TILE
    chain = [m["chain_start"] + i * m["slen"] for i in range(m["chain_frames"])]
    chain = [o for o in chain if lo <= o < m["host_end"]]
    first = m["pre_frames"] + 1
    real = [int(ref["payload_off"][i]) - 2 for i in range(first, ref["nframes"])]  # (C2: 2 header bytes)
    return chain, [o for o in real if o < hi]


def check_site(decoder, wire, m, kind, records=True):
    ref = O.decode_batch(wire)
    pre, post, n, cs, he = m["pre_frames"], m["post_frames"], m["chain_frames"], m["chain_start"], m["host_end"]
    # the real framing: pre C2 frames, the host, post C2 frames
    assert ref["err_code"] == 0 and ref["tail"] == 0 and ref["nframes"] == pre + 1 + post
    off, ln = ref["payload_off"].astype(np.int64), ref["payload_len"].astype(np.int64)
    np.testing.assert_array_equal(off[:pre], np.arange(pre) * 86 + 2)
    assert off[pre] > m["host_start"] and off[pre] + ln[pre] == he and m["end"] == len(wire)
    np.testing.assert_array_equal(off[pre + 1:], he + np.arange(post) * 86 + 2)
    # the merge: from the chain's first header, its frames and then the real frames after the host
    d = O.decode_batch(wire[cs:])
    assert d["err_code"] == 0 and d["nframes"] == n + post
    np.testing.assert_array_equal(d["payload_off"][:n].astype(np.int64), np.arange(n) * m["slen"] + 2)
    assert (d["payload_len"][:n] == m["slen"] - 2).all() and (d["type"][:n] == ID[kind]).all()
    np.testing.assert_array_equal(d["payload_off"][n:].astype(np.int64) + cs, off[pre + 1:])
    for c in ["payload_len", "type"] + COLS:
        np.testing.assert_array_equal(d[c][n:], ref[c][pre + 1:], err_msg=c)
    # geometry
    t, k = m["t"], m["k"]
    assert he // S.TILE == t and he % S.TILE // S.SEG == k
    hdr = np.concatenate([off[:pre] - 2, [m["host_start"]], off[pre + 1:] - 2])
    assert not ((hdr >= (t - 1) * S.TILE) & (hdr < t * S.TILE)).any()
    assert m["host_start"] // S.TILE == t - 1 - m["whole_tiles"]
    assert 24 <= cs - int(off[pre]) - (ref["value_off"][pre] if ref["type"][pre] == 1 else 0) < 24 + m["slen"]
    chain, real = tile_frames(wire, m, ref)
    if k >= 2:
        assert chain
    if m["slen"] > S.SEG:  # the entry is the first header of its segment
        assert not chain or chain[-1] // S.SEG < he // S.SEG
    assert (len(chain) + len(real) <= CR_CAP) == records
    # every frame of tile t in the record's shape
    recs = run(decoder, wire, [(o, ID[kind], 0) for o in chain] + [(o, 1, 0) for o in real])
    assert all(r[0] == 1 for r in recs), [r for r in recs if r[0] != 1][:3]
    if kind == "wide":  # five-word records: a number of 2^10 or more
        assert all(max(r[5:8]) >= 2 ** 10 for r in recs[:len(chain)])
    if kind == "narrow":
        assert all(max(r[5:8]) < 2 ** 10 for r in recs[:len(chain)])
    return len(chain), len(real)


@pytest.mark.parametrize("whole_tiles", [1, 2])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("kind", S.SITE_KINDS)
@pytest.mark.parametrize("host", S.SITE_HOSTS)
def test_site_merges(decoder, host, kind, k, whole_tiles):
    wire, m = S.merge_site(PRE, k, SLEN, kind, host, whole_tiles, POST, seed=31 + k)
    nc, nr = check_site(decoder, wire, m, kind)
    # 100-byte chain frames, the host's end 7 bytes into segment k, 86-byte frames after it
    assert (nc, nr) == {1: (0, 95), 2: (1, 94), 63: (40, 49), 64: (41, 48), 65: (41, 47), 127: (81, 1)}[k]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("host", S.SITE_HOSTS)
def test_site_header_at_tile_end(decoder, host, k):
    """95 C2 frames end 22 bytes before a tile's end: the host's header is its tile's last frame and
    the chain starts in the next tile (the header's tile holds the real framing only)."""
    wire, m = S.merge_site(95, k, SLEN, "narrow", host, 1, POST, seed=31 + k)
    check_site(decoder, wire, m, "narrow")
    assert m["host_start"] % S.TILE == S.TILE - 22 and m["chain_start"] // S.TILE == m["t"] - 1


@pytest.mark.parametrize("kind", ["blob", "narrow"])
def test_no_records_control(decoder, kind):
    """40-byte chain frames: tile t holds more than 128 frames, so claims_fast keeps no records of it."""
    wire, m = S.merge_site(PRE, 127, 40, kind, "blob", 1, POST, seed=5)
    nc, nr = check_site(decoder, wire, m, kind, records=False)
    assert nc + nr > CR_CAP


def test_filler_control():
    """chain=False: the same real frames, random bytes where the chain was."""
    a, ma = S.merge_site(PRE, 64, SLEN, "narrow", "blob", 1, POST, seed=9)
    b, mb = S.merge_site(PRE, 64, SLEN, "narrow", "blob", 1, POST, seed=9, chain=False)
    assert ma == mb and len(a) == len(b) and a != b
    cs, he = ma["chain_start"], ma["host_end"]
    assert a[:cs] == b[:cs] and a[he:] == b[he:]
    ra, rb = O.decode_batch(a), O.decode_batch(b)
    for c in ["payload_off", "payload_len", "type"] + COLS:
        np.testing.assert_array_equal(ra[c], rb[c], err_msg=c)


def test_cascade_composition():
    """Sites, a never-merging segment on a frame boundary, a site behind it: the oracle decodes the
    whole wire, every site's tile t is where its meta says, and the segment's frames follow the
    frames before it."""
    site = dict(pre_frames=PRE, k=64, slen=SLEN, kind="narrow", host="blob", whole_tiles=1, post_frames=POST)
    wire, metas = S.site_cascade([site, dict(site, k=2, host="change")], shadow_n=6, after=[dict(site, k=127)])
    ref = O.decode_batch(wire)
    assert ref["err_code"] == 0 and ref["tail"] == 0
    assert ref["nframes"] == 3 * (PRE + 1 + POST) + 6 + 300 + 300
    ends = ref["payload_off"].astype(np.int64) + ref["payload_len"].astype(np.int64)
    a, b = metas[0]["shadow"]
    assert a in ends and b in ends and a % S.TILE != 0
    for m in metas:
        assert m["host_end"] in ends and m["host_end"] // S.TILE == m["t"]
    assert metas[0]["t"] < metas[1]["t"] < a // S.TILE < b // S.TILE < metas[2]["t"]
