"""GPU parity for the latest-per-key compaction: drp_latest_device (of the rows the select predicate
keeps, the one with the greatest change per (subset presence, subset bytes, key bytes), the later
row on a tie, in row order) and drp_latest_staged (that step between select and encode over the
staged batch). Every comparison is bit-exact against an expected side built here on the CPU: the
oracle's decode of the wire, the select predicate in numpy, a dict from identity to the best
(change, row), and the oracle's encoding of the winners in row order."""
import ctypes as C
import random

import numpy as np
import pytest

import _oracle as O
import _streams as S
from _relay import (SRC_KEYS, U64MAX, check_decoded as _check_decoded, make_filter as _filter, mask as _mask,
                    rows as _rows, winners as _winners)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from _gpu import drp_amd
    c = drp_amd.Ctx(0)
    c.set_blob_skip(drp_amd.BLOB_SKIP_OFF)
    yield c
    c.close()


# ---- the expected side (the predicate, the winners, the rows and the decoded check: _relay) ---

def _expected(wire, spec, blob_remaining=0):
    w = np.frombuffer(wire, np.uint8)
    ref = O.decode_batch(wire, blob_remaining=blob_remaining)
    n = ref["nframes"]  # delivered rows only: nothing at or after an error frame
    idx, best = _winners(w, ref, np.flatnonzero(_mask(w, ref, n, spec)))
    cols = _rows(ref, idx)
    return O.encode_changes(wire, cols), idx, cols, ref, best


def _latest(ctx, wire, spec, blob_remaining=0, stage=None):
    """Stage `wire` (or the chunk list `stage` that spells it), run drp_latest_staged and compare
    with the expected side, bytes and decoded fields."""
    want, idx, cols, ref, _ = _expected(wire, spec, blob_remaining)
    g = ctx.decode_staged(stage if stage is not None else wire, blob_remaining=blob_remaining)
    assert g["nframes"] == ref["nframes"] and g["err_code"] == ref["err_code"]
    out, nsel = ctx.latest_staged(_filter(spec))
    assert nsel == len(idx), (spec, nsel, len(idx))
    assert out == want, (spec, len(out), len(want))
    _check_decoded(out, wire, cols)
    return out, idx


def _wire(rows):
    """rows: (key, subset or None, change); from / to / value tell the rows of a key apart."""
    return b"".join(S.frame(S.change_payload(k, ch, r % 128, (r * 7) % 128, value=b"%d" % r if r % 3 else None,
                                             subset=sub)) for r, (k, sub, ch) in enumerate(rows))


def _pool_rows(n, pool, changes, seed, subsets=(None,)):
    rng = random.Random(seed)
    return [(b"key-%d" % rng.randrange(pool), rng.choice(subsets), rng.randrange(changes)) for _ in range(n)]


# ---- row counts ------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_row_counts(ctx, n):
    """0, 1 and the wave (64) and workgroup (1024) sizes, one row below, at and above; keys from a
    pool of n // 4, changes from a range of 5, so every key repeats and ties occur."""
    rows = _pool_rows(n, max(1, n // 4), 5, seed=n, subsets=(None, None, b"s"))
    out, idx = _latest(ctx, _wire(rows), {})
    if n >= 63:
        assert 0 < len(idx) < n
        by_key = {}
        for r, (k, sub, ch) in enumerate(rows):
            by_key.setdefault((k, sub, ch), []).append(r)
        assert any(len(v) > 1 for v in by_key.values())  # (ties were there to break)


# ---- contention, distinctness, ties ----------------------------------------------------------

def test_one_key_everywhere(ctx):
    """2049 rows of one key: one row out, the last of those with the greatest change."""
    rng = random.Random(1)
    rows = [(b"hot", None, rng.randrange(7)) for _ in range(2049)]
    out, idx = _latest(ctx, _wire(rows), {})
    last = max(r for r, (_, _, ch) in enumerate(rows) if ch == 6)
    assert list(idx) == [last]


def test_all_keys_distinct(ctx):
    """No key repeats: the bytes are drp_relay_staged's with the same filter."""
    rows = [(b"k%05d" % r, None, r % 9) for r in range(2049)]
    wire = _wire(rows)
    for spec in [{}, {"change_range": (2, 5)}]:
        out, idx = _latest(ctx, wire, spec)
        assert ctx.relay_staged(_filter(spec))[0] == out
    assert len(_latest(ctx, wire, {})[1]) == 2049


def test_one_key_one_change(ctx):
    """Every row the same key and the same change: the last row wins."""
    out, idx = _latest(ctx, _wire([(b"same", b"sub", 42)] * 2049), {})
    assert list(idx) == [2048]


# ---- identity edges --------------------------------------------------------------------------

def test_identity_edges(ctx):
    """Keys that are prefixes of one another and the empty key; one key under an absent, an empty
    and two one-byte subsets; key + subset concatenations that are equal but split differently."""
    keys = [b"", b"a", b"ab", b"a\x00"]
    subs = [None, b"", b"s", b"t"]
    rows = []
    for rep in range(3):
        rows += [(k, None, 10 + rep) for k in keys]
        rows += [(b"same", sub, 20 - rep) for sub in subs]
        rows += [(b"ab", b"c", 5 + rep), (b"a", b"bc", 7 - rep), (b"abc", b"", 1), (b"", b"abc", 2)]
    out, idx = _latest(ctx, _wire(rows), {})
    assert len(idx) == len(keys) + len(subs) + 4
    per = len(keys) + len(subs) + 4
    # rising changes: the last repetition's row; falling ones: the first's; equal ones: the last's
    assert list(idx) == sorted([2 * per + k for k in range(4)] + [4 + k for k in range(4)] +
                               [2 * per + 8, 9, 2 * per + 10, 2 * per + 11])


def test_change_extremes(ctx):
    """0, 1, 2^63 and 2^64 - 1 within one group (unsigned compare), and a group whose only value
    is 0 (the table's cleared word equals it)."""
    rows = [(b"big", None, 2**63), (b"zero", None, 0), (b"big", None, U64MAX), (b"big", None, 1), (b"big", None, 0),
            (b"zero", None, 0), (b"mid", None, 2**63), (b"mid", None, 2**63 - 1), (b"big", None, 2**63)]
    out, idx = _latest(ctx, _wire(rows), {})
    assert list(idx) == [2, 5, 6]


# ---- hash mask -------------------------------------------------------------------------------

def test_hash_mask(ctx):
    """300 rows over 40 identities with the row hash cut to 0, 1 and 3 bits and whole: mask 0
    sends every row to one start slot, a 40-long probe chain whose every step compares the rows;
    the bytes never change."""
    rng = random.Random(40)
    idents = [(b"key%02d" % (k // 2), None if k % 2 else b"x") for k in range(40)]
    rows = [(*idents[k], 0) for k in range(40)] + [(*rng.choice(idents), rng.randrange(6)) for _ in range(260)]
    wire = _wire(rows)
    want, idx, _, _, best = _expected(wire, {})
    assert len(best) == 40
    try:
        outs = []
        for mask in [0, 1, 7, U64MAX]:
            ctx.set_latest_hash_mask(mask)
            outs.append(_latest(ctx, wire, {})[0])
        assert outs == [want] * 4
    finally:
        ctx.set_latest_hash_mask(U64MAX)


def test_long_keys_differ_in_one_byte(ctx):
    """Keys and subsets of 7, 8, 9, 15, 16, 17 and 40 bytes (the byte compare takes eight at a
    time from 8 on, the last eight overlapping) that differ in the first, a middle or the last
    byte only, with the hash cut to nothing so that every probe step compares bytes."""
    idents = []
    for n in [7, 8, 9, 15, 16, 17, 40]:
        base = bytes(range(65, 65 + n))
        for pos in [None, 0, n // 2, n - 1]:
            k = base if pos is None else base[:pos] + b"!" + base[pos + 1:]
            idents += [(k, None), (b"k", k)]
    assert len(set(idents)) == len(idents) == 56
    rng = random.Random(3)
    rows = [(*idents[k], 1) for k in range(56)] + [(*rng.choice(idents), rng.randrange(4)) for _ in range(400)]
    wire = _wire(rows)
    want, idx, _, _, best = _expected(wire, {})
    assert len(best) == 56
    try:
        for mask in [0, U64MAX]:
            ctx.set_latest_hash_mask(mask)
            assert _latest(ctx, wire, {})[0] == want
    finally:
        ctx.set_latest_hash_mask(U64MAX)


# ---- filters ---------------------------------------------------------------------------------

def test_snapshot_is_not_latest_then_filter(ctx):
    """change <= T gives every key's state at T: a key whose latest change is beyond T still
    shows its last change up to T. Filtering the unfiltered result would drop it."""
    rows = _pool_rows(600, 50, 20, seed=5, subsets=(None, b"s"))
    wire = _wire(rows)
    t = 9
    snap, idx = _latest(ctx, wire, {"change_range": (0, t)})
    full_want, full_idx, _, ref, _ = _expected(wire, {})
    then_filter = full_idx[ref["change"][full_idx] <= np.uint64(t)]
    assert len(then_filter) < len(idx)
    assert snap != O.encode_changes(wire, _rows(ref, then_filter))
    assert np.all(ref["change"][idx] <= np.uint64(t)) and np.any(ref["change"][full_idx] > np.uint64(t))


def test_filters(ctx):
    """A key prefix, subset_none, a subset, conditions combined, and an empty result."""
    rows = _pool_rows(700, 60, 6, seed=6, subsets=(None, b"s", b"tt", b""))
    wire = _wire(rows)
    counts = {}
    for name, spec in {"prefix": {"key_prefix": b"key-1"}, "none": {"subset_none": True}, "sub": {"subset": b"tt"},
                       "both": {"key_prefix": b"key-2", "subset": b"", "change_range": (1, 4)},
                       "empty": {"key_prefix": b"nothing"}, "empty2": {"change_range": (7, 3)}}.items():
        counts[name] = len(_latest(ctx, wire, spec)[1])
    assert counts["empty"] == 0 and counts["empty2"] == 0
    assert counts["prefix"] > 4 and counts["none"] > 4 and counts["sub"] > 4 and counts["both"] > 0


# ---- frames around the Changes ---------------------------------------------------------------

def _with_blobs(rows, every=37, blob_len=900, seed=2):
    rng = random.Random(seed)
    parts = []
    for r, (k, sub, ch) in enumerate(rows):
        if r % every == every - 1:
            parts.append(S.frame(rng.randbytes(blob_len), 2))
        parts.append(S.frame(S.change_payload(k, ch, r % 128, 3, value=b"%d" % r, subset=sub)))
    return b"".join(parts)


def test_blobs_and_batch_edges(ctx):
    """Blobs between the Changes; a batch that starts inside a blob (an odd length: the staged
    bytes are shifted against the batch offsets)."""
    body = _with_blobs(_pool_rows(500, 40, 5, seed=7, subsets=(None, b"s")))
    plain = _latest(ctx, body, {})[0]
    for brem in [1000, 5]:
        wire = random.Random(brem).randbytes(brem) + body
        assert _latest(ctx, wire, {}, blob_remaining=brem)[0] == plain
        _latest(ctx, wire, {"key_prefix": b"key-3"}, blob_remaining=brem)


def test_error_ends_the_rows(ctx):
    """A type >= 3 mid-way: nothing at or after the error frame takes part, so a key's later and
    greater change behind it does not win. A malformed Change: it is the last row and no candidate."""
    a = _pool_rows(200, 20, 5, seed=8)
    b = [(k, sub, ch + 100) for k, sub, ch in _pool_rows(50, 20, 5, seed=9)]
    wa, wb = _wire(a), _wire(b)
    for mid, code in [(b"\x03\x07ab", 1), (S.frame(b"\x12\x05ab"), 4)]:
        wire = wa + mid + wb
        assert O.decode_batch(wire)["err_code"] == code
        out, idx = _latest(ctx, wire, {})
        assert out == _expected(wa, {})[0] and len(idx) and idx.max() < 200


def _blob_stream():
    """Units of 150 Changes over a small key pool and one 300 KB blob, long enough for the stage
    step to cut it into pieces that skip blob payload; the keys repeat across the pieces."""
    rng = random.Random(11)
    parts = []
    for u in range(5):
        parts.append(_wire([(k, sub, ch + u) for k, sub, ch in _pool_rows(150, 60, 4, seed=20 + u, subsets=(None, b"s"))]))
        parts.append(S.frame(rng.randbytes(300000), 2))
    return b"".join(parts)


def test_blob_skip_modes_and_chunks(ctx):
    """The same bytes with the batch staged whole and in blob-skipping pieces (the piece table
    reaches the grouping kernels: a slot's row lies in another piece than the row that visits it),
    and with the batch given as a list of chunks."""
    from _gpu import drp_amd
    big = _blob_stream()
    assert len(big) > 1 << 20
    chunks = [big[i:i + 100003] for i in range(0, len(big), 100003)]
    try:
        for spec in [{}, {"change_range": (0, 4)}, {"key_prefix": b"key-1", "subset": b"s"}]:
            outs = []
            for mode in [drp_amd.BLOB_SKIP_OFF, drp_amd.BLOB_SKIP_ALWAYS]:
                ctx.set_blob_skip(mode)
                outs.append(_latest(ctx, big, spec)[0])
                if mode == drp_amd.BLOB_SKIP_ALWAYS:
                    assert ctx.timing().h2d_skipped > 0  # (it was staged in pieces)
                outs.append(_latest(ctx, big, spec, stage=chunks)[0])
            assert outs[1:] == outs[:1] * 3
    finally:
        ctx.set_blob_skip(drp_amd.BLOB_SKIP_OFF)


# ---- drp_latest_device -----------------------------------------------------------------------

def test_latest_device_multi_stream(ctx):
    """drp_latest_device over the flat output of one drp_decode_device call for three streams that
    share keys: sel_idx, n_selected and the encoder rows against the expected side over the
    streams' rows end to end; across streams the later stream wins a tie."""
    import torch
    from _gpu import drp_amd
    dev = torch.device("cuda", 0)
    shared = [(b"tie", None, 5), (b"tie2", b"s", 0)]
    third = _pool_rows(1300, 90, 6, seed=33, subsets=(None, b"s"))
    streams = [_wire(_pool_rows(700, 90, 6, seed=31, subsets=(None, b"s")) + shared),
               _wire(shared + _pool_rows(90, 90, 6, seed=32, subsets=(None, b"s"))),
               _wire(third[:650] + shared + third[650:])]
    offs = np.concatenate([[0], np.cumsum([len(w) for w in streams])]).astype(np.int64)
    wire = b"".join(streams)
    w = np.frombuffer(wire, np.uint8)
    wire_t = torch.from_numpy(w.copy()).to(dev)
    so_t, en_t = torch.from_numpy(offs).to(dev), torch.zeros(3, dtype=torch.int64, device=dev)
    cap = len(wire) // 2 + 64
    outs = {"payload_off": torch.zeros(cap, dtype=torch.int64, device=dev),
            "payload_len": torch.zeros(cap, dtype=torch.int32, device=dev),
            "type": torch.zeros(cap, dtype=torch.uint8, device=dev),
            "flags": torch.zeros(cap, dtype=torch.uint8, device=dev)}
    for k in drp_amd.COLS32:
        outs[k] = torch.zeros(cap, dtype=torch.int32, device=dev)
    for k in drp_amd.COLS64:
        outs[k] = torch.zeros(cap, dtype=torch.int64, device=dev)
    rs = C.sizeof(drp_amd.StreamResult)
    res_t = torch.zeros(3 * rs, dtype=torch.uint8, device=dev)
    ctx.decode_device(wire_t, so_t, en_t, outs, cap, res_t)
    raw = res_t.cpu().numpy().tobytes()
    res = [drp_amd.StreamResult.from_buffer_copy(raw[s * rs:(s + 1) * rs]) for s in range(3)]
    n = sum(r.frames for r in res)
    # the expected side: the streams' oracle rows end to end, payload offsets into the whole wire
    refs = [O.decode_batch(s) for s in streams]
    assert [r.frames for r in res] == [r["nframes"] for r in refs] and n == 700 + 90 + 1300 + 6
    ref = {k: np.concatenate([r[k][:r["nframes"]] for r in refs]) for k in
           ["type", "flags"] + O.COLS32 + O.COLS64}
    ref["payload_off"] = np.concatenate([r["payload_off"][:r["nframes"]] + np.uint64(offs[s])
                                         for s, r in enumerate(refs)])
    for spec in [{}, {"change_range": (0, 5)}, {"subset_none": True, "key_prefix": b"key-1"}]:
        want_idx, best = _winners(w, ref, np.flatnonzero(_mask(w, ref, n, spec)))
        want = _rows(ref, want_idx)
        rows = {k: torch.full((n,), 0x55, dtype=(torch.int32 if k.endswith("_len") else
                                                torch.uint8 if k == "flags" else torch.int64), device=dev)
                for k in SRC_KEYS}
        idx_t = torch.full((n,), -1, dtype=torch.int64, device=dev)
        nsel_t = torch.full((1,), -1, dtype=torch.int64, device=dev)
        ctx.latest_device(wire_t, outs, n, _filter(spec), rows, idx_t, nsel_t)
        torch.cuda.synchronize()
        nsel = int(nsel_t.cpu()[0])
        assert nsel == len(want_idx) and 0 < nsel < n
        sel_idx = idx_t.cpu().numpy()
        np.testing.assert_array_equal(sel_idx[:nsel], want_idx)
        assert np.all(sel_idx[nsel:] == -1)
        for k in SRC_KEYS:
            got = rows[k].cpu().numpy()
            np.testing.assert_array_equal(got[:nsel].astype(want[k].dtype), want[k], err_msg=k)
            assert np.all(got[nsel:] == 0x55), k  # nothing past the winners
        # the rows encode on the device, with the wire as the heap, to the oracle's bytes
        foff_t = torch.zeros(nsel + 1, dtype=torch.int64, device=dev)
        out_t = torch.zeros(len(wire), dtype=torch.uint8, device=dev)
        ctx.encode_device(rows, wire_t, nsel, foff_t, out_t, len(wire))
        torch.cuda.synchronize()
        total = int(foff_t.cpu()[nsel])
        assert out_t.cpu().numpy()[:total].tobytes() == O.encode_changes(wire, want)
        if not spec:  # the shared rows tie across the streams: the third stream's copy wins
            begin3 = res[2].frame_begin
            assert best[(False, b"", b"tie")][1] >= begin3 and best[(True, b"s", b"tie2")][1] >= begin3
    # without sel_idx
    nsel_t.fill_(-1)
    ctx.latest_device(wire_t, outs, n, None, rows, None, nsel_t)
    torch.cuda.synchronize()
    assert int(nsel_t.cpu()[0]) == len(_winners(w, ref, np.flatnonzero(_mask(w, ref, n, {})))[0])


# ---- error returns, determinism --------------------------------------------------------------

@pytest.fixture(scope="module")
def mixed():
    return _with_blobs(_pool_rows(800, 70, 6, seed=12, subsets=(None, b"s", b"")))


def test_capacity(ctx, mixed):
    """cap one byte short: DRP_E_CAPACITY, .written = the size needed, out keeps its fill."""
    from _gpu import drp_amd
    want, idx, _, _, _ = _expected(mixed, {})
    ctx.decode_staged(mixed)
    need = len(want)
    buf = np.full(need + 64, 0xAB, np.uint8)
    with pytest.raises(drp_amd.DrpError) as e:
        ctx.latest_staged(None, cap=need - 1, out=buf)
    assert e.value.rc == drp_amd.DRP_E_CAPACITY and e.value.written == need
    assert np.all(buf == 0xAB)
    out, nsel = ctx.latest_staged(None, cap=need, out=buf)
    assert out == want and nsel == len(idx) and np.all(buf[need:] == 0xAB)


def test_invalid_arguments(ctx, mixed):
    """A bad filter, no staged batch, and a staged batch a host encode has ended: DRP_E_INVAL; the
    rows can still be fetched after a call."""
    from _gpu import drp_amd
    want, idx, cols, ref, _ = _expected(mixed, {})
    ctx.decode_staged(mixed)
    for f in [drp_amd.make_filter(flags=0x10), drp_amd.make_filter(subset=b"a", subset_none=True),
              drp_amd.make_filter(key_prefix=bytes(257))]:
        with pytest.raises(drp_amd.DrpError) as e:
            ctx.latest_staged(f)
        assert e.value.rc == drp_amd.DRP_E_INVAL
    with drp_amd.Ctx(0) as fresh:  # nothing staged yet
        with pytest.raises(drp_amd.DrpError) as e:
            fresh.latest_staged(None)
        assert e.value.rc == drp_amd.DRP_E_INVAL
    assert ctx.latest_staged(None)[0] == want
    # fetch still works after a call
    rows = len(ref["type"])
    o = drp_amd.alloc_host_outputs(rows)
    fr, co = drp_amd._structs(o, drp_amd._p)
    assert ctx.L.drp_decode_fetch(ctx.h, C.byref(fr), C.byref(co), 0, rows) == 0
    for k in ["payload_off", "payload_len", "type"]:
        np.testing.assert_array_equal(o[k], ref[k][:rows], err_msg=k)
    ch = (ref["type"][:rows] & 0x3F) == 1
    for k in O.COLS32 + O.COLS64 + ["flags"]:
        np.testing.assert_array_equal(o[k][ch], ref[k][:rows][ch], err_msg=k)
    # a host encode takes the staging the wire lives in
    assert ctx.encode_batch(np.frombuffer(mixed * 3, np.uint8), cols) == want
    with pytest.raises(drp_amd.DrpError) as e:
        ctx.latest_staged(None)
    assert e.value.rc == drp_amd.DRP_E_INVAL
    ctx.decode_staged(mixed)
    assert ctx.latest_staged(None)[0] == want


def test_deterministic(ctx, mixed):
    """The same call twice, and again after a drp_relay_staged in between (they share the
    scratch): identical bytes."""
    want, idx, _, _, _ = _expected(mixed, {})
    ctx.decode_staged(mixed)
    first = ctx.latest_staged(None)
    assert first == (want, len(idx)) and ctx.latest_staged(None) == first
    relayed = ctx.relay_staged(None)
    assert relayed[1] == 800 and ctx.latest_staged(None) == first
    assert ctx.relay_staged(None) == relayed
