"""GPU parity for the relay path: drp_select_device (predicate + stable compaction of decoded
Changes into encoder rows) and drp_relay_staged (select over the staged batch, then the encoder
with the staged wire as its heap). Every comparison is bit-exact against the CPU oracle: decode
the wire, apply the predicate in numpy, make the kept rows' offsets absolute, encode them."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest

import _oracle as O
import _streams as S
from _relay import (SRC_KEYS, U64MAX, bytes_at as _bytes_at, check_decoded as _check_decoded, make_filter as _filter,
                    mask as _mask, rows as _rows)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    from _gpu import drp_amd
    c = drp_amd.Ctx(0)
    c.set_blob_skip(drp_amd.BLOB_SKIP_OFF)
    yield c
    c.close()


# ---- the expected side (the predicate, the rows and the decoded check: _relay) ---------------

def _expected(wire, spec, blob_remaining=0):
    w = np.frombuffer(wire, np.uint8)
    ref = O.decode_batch(wire, blob_remaining=blob_remaining)
    n = ref["nframes"]  # delivered rows only: nothing at or after an error frame
    idx = np.flatnonzero(_mask(w, ref, n, spec))
    cols = _rows(ref, idx)
    return O.encode_changes(wire, cols), idx, cols, ref


def _relay(ctx, wire, spec, blob_remaining=0, decoded=True, **stage_kw):
    want, idx, cols, ref = _expected(wire, spec, blob_remaining)
    g = ctx.decode_staged(wire, blob_remaining=blob_remaining, **stage_kw)
    assert g["nframes"] == ref["nframes"] and g["err_code"] == ref["err_code"]
    out, nsel = ctx.relay_staged(_filter(spec))
    assert nsel == len(idx), (spec, nsel, len(idx))
    assert out == want, (spec, len(out), len(want))
    if decoded:
        _check_decoded(out, wire, cols)
    return out, idx


# ---- row counts x selections -----------------------------------------------------------------

def _c2_specs(n):
    first = b"%010d" % 0
    last = b"%010d" % max(n - 1, 0)
    return {"all": {}, "none": {"change_range": (1000, 2000)}, "half": {"change_range": (0, 50)},
            "first": {"key_prefix": first}, "last": {"key_prefix": last}}


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 2 * 1024 + 1])
def test_row_counts(ctx, n):
    """0, 1 and the wave (64) and workgroup (1024) sizes, one row below, at and above: all rows,
    none, the half with change <= 50, only the first and only the last row."""
    wire = S.c2_stream(n, seed=3).tobytes()
    for name, spec in _c2_specs(n).items():
        out, idx = _relay(ctx, wire, spec, decoded=n <= 65)
        want_n = {"all": n, "none": 0, "half": sum(1 for i in range(n) if i % 100 < 50),
                  "first": min(n, 1), "last": min(n, 1)}[name]
        assert len(idx) == want_n, (name, len(idx))
        if name == "last" and n:
            assert idx[0] == n - 1


def test_rows_past_one_scan_round(ctx):
    """1024 * 1024 + 1 rows, staged once: the scan of the workgroup counts takes a second round
    with a carry (1024 counts per round). All five selections: every workgroup's count full
    (all), a zero total across the rounds (none), the half with change <= 50, only the first row,
    and only the last row (every count zero but the second round's only workgroup). The kept
    rows are the C2 stream's closed form (change = i % 100 + 1, key = the 10 digits of i), checked
    against the oracle's columns; the bytes are the oracle's encoding of those rows."""
    n = 1024 * 1024 + 1
    wire = S.c2_stream(n, seed=4).tobytes()
    w = np.frombuffer(wire, np.uint8)
    ref = O.decode_batch(wire, cap=n + 8)
    assert ref["nframes"] == n and ref["err_code"] == 0
    i = np.arange(n)
    np.testing.assert_array_equal(ref["change"][:n], (i % 100 + 1).astype(np.uint64))
    assert np.all(ref["key_len"][:n] == 10) and np.all(ref["type"][:n] == 1) and not np.any(ref["flags"][:n] & 4)
    specs = _c2_specs(n)
    for r in (0, n - 1):  # the two prefixes are those rows' whole keys (and no other row's: distinct numbers)
        off = int(ref["payload_off"][r]) + int(ref["key_off"][r])
        assert _bytes_at(w, off, 10) == specs["first" if r == 0 else "last"]["key_prefix"]
    keep = {"all": i, "none": i[:0], "half": np.flatnonzero(i % 100 < 50), "first": i[:1], "last": i[-1:]}
    assert len(keep["half"]) == (n // 100) * 50 + min(n % 100, 50)
    g = ctx.decode_staged(wire)
    assert g["nframes"] == n
    for name, spec in specs.items():
        want = O.encode_changes(wire, _rows(ref, keep[name]))
        out, nsel = ctx.relay_staged(_filter(spec))
        assert nsel == len(keep[name]), (name, nsel)
        assert out == want, name


# ---- mixed content, every condition ----------------------------------------------------------

def _crafted():
    """Frames around every edge of the byte conditions: subsets absent / empty / equal length with
    a different last byte / 255 and 256 bytes, keys empty / a prefix of one another."""
    s255, s256 = bytes(range(255)), bytes(range(256))
    s256b = s256[:-1] + b"\x00"
    rows = [
        (b"", None, 7), (b"", b"", 8), (b"k", b"abc", 9), (b"key", b"abd", 10), (b"key1", b"abc", 11),
        (b"key12", s255, 12), (b"key", s256, 13), (b"ke", s256b, 14), (b"x" * 300, b"", 15),
        (b"key1", None, 2**53 - 1), (b"zz", s255[:-1] + b"\x01", 16), (b"key", b"abc", 11),
    ]
    return b"".join(S.frame(S.change_payload(k, ch, 1, 2, value=b"v" * (ch % 5), subset=sub))
                    for k, sub, ch in rows)


@pytest.fixture(scope="module")
def mixed():
    return S.random_stream_seeded(5, 300) + _crafted() + S.random_stream_seeded(6, 300)


def _mixed_specs(wire):
    ref = O.decode_batch(wire)
    n = ref["nframes"]
    ch = ref["change"][:n][(ref["type"][:n] & 0x3F) == 1]
    v = int(np.sort(ch)[len(ch) // 2])  # a value that is present
    s255, s256 = bytes(range(255)), bytes(range(256))
    specs = [
        {},
        {"change_range": (v, v)}, {"change_range": (v + 1, U64MAX)}, {"change_range": (0, v - 1)},
        {"change_range": (v, U64MAX)}, {"change_range": (0, v)}, {"change_range": (v + 1, v)},
        {"change_range": (2**53 - 1, 2**53 - 1)}, {"change_range": (0, U64MAX)},
        {"subset": b""}, {"subset_none": True},
        {"subset": b"abc"}, {"subset": b"abd"}, {"subset": b"abe"},
        {"subset": s255}, {"subset": s256}, {"subset": s256[:-1] + b"\x00"}, {"subset": s256[:-1] + b"\x07"},
        {"key_prefix": b""}, {"key_prefix": b"key"}, {"key_prefix": b"key1"}, {"key_prefix": b"key123"},
        {"key_prefix": b"x" * 256}, {"key_prefix": b"x" * 255 + b"y"},
        {"key_prefix": b"key", "subset": b"abc", "change_range": (11, 11)},
        {"key_prefix": b"key1", "subset_none": True, "change_range": (0, 2**53)},
        {"key_prefix": b"a", "change_range": (0, 2**32)},
    ]
    return specs


def test_mixed_content_every_condition(ctx, mixed):
    """Blobs, id-0 headers, subsets, big keys and numbers up to 2^53 - 1, with no filter and with
    each condition: range bounds on a present value and one off it, min > max; subset present
    and empty against absent (SUBSET_EQ length 0, SUBSET_NONE), equal length with a different last
    byte, lengths 255 and 256; key prefix longer than the key, the whole key, length 0 and
    key_len == 0; and conditions combined."""
    hits = {}
    for spec in _mixed_specs(mixed):
        out, idx = _relay(ctx, mixed, spec)
        hits[json.dumps({k: (v.hex() if isinstance(v, bytes) else v) for k, v in spec.items()})] = len(idx)
    # the crafted rows make these selections non-trivial
    assert hits[json.dumps({"subset": bytes(range(256)).hex()})] == 1
    assert hits[json.dumps({"subset": bytes(range(255)).hex()})] == 1
    assert hits[json.dumps({"subset": b"abc".hex()})] >= 3
    assert hits[json.dumps({"key_prefix": (b"x" * 256).hex()})] == 1
    assert hits[json.dumps({"key_prefix": (b"x" * 255 + b"y").hex()})] == 0
    assert hits[json.dumps({"key_prefix": b"key".hex(), "subset": b"abc".hex(), "change_range": [11, 11]})] == 2


def test_non_canonical_payloads(ctx):
    """Overlong varints, reordered and duplicate fields (tests/golden/change_codec.json) come out
    as the canonical encoding: the oracle's, which is also messages.Change.encode of the fields."""
    vec = json.load(open(os.path.join(ROOT, "tests", "golden", "change_codec.json")))["vectors"]
    assert any(not v["canonical"] for v in vec)
    wire = b"".join(S.frame(bytes.fromhex(v["payload"])) for v in vec)
    out, idx = _relay(ctx, wire, {})
    assert len(idx) == len(vec)
    canon = b"".join(S.frame(O.change_encode(bytes.fromhex(v["subset"]) if v["has_subset"] else None,
                                             bytes.fromhex(v["key"]), v["change"], v["from"], v["to"],
                                             bytes.fromhex(v["value"]) if v["has_value"] else None)) for v in vec)
    assert out == canon


# ---- errors, batch edges, modes --------------------------------------------------------------

@pytest.mark.parametrize("bad", ["type", "change", "required"])
def test_error_in_the_stream(ctx, bad):
    """An error mid-way (a type >= 3, a malformed Change, a Change without its key): nothing at
    or after the error frame is relayed, the DRP_F_BAD row included."""
    a, b = S.random_stream_seeded(7, 120), S.random_stream_seeded(8, 50)
    mid = {"type": b"\x03\x07ab", "change": S.frame(b"\x12\x05ab"),
           "required": S.frame(b"\x18\x01\x20\x02\x28\x03")}[bad]
    wire = a + mid + b
    ref = O.decode_batch(wire)
    assert ref["err_code"] == {"type": 1, "change": 4, "required": 5}[bad]
    assert ref["nframes"] == O.decode_batch(a)["nframes"]
    for spec in [{}, {"key_prefix": b""}, {"change_range": (0, 2**40)}]:
        out, idx = _relay(ctx, wire, spec)
        assert out == _expected(a, spec)[0]


def test_batch_edges(ctx):
    """A batch that starts inside a blob (blob_remaining > 0, an odd length: the staged bytes are
    shifted against the batch offsets), one that ends in a partial blob, one that ends inside a
    Change: only the delivered Changes are relayed."""
    body = S.random_stream_seeded(9, 200)
    changes = _expected(body, {})[0]
    for brem in [1000, 16, 5]:
        wire = random.Random(brem).randbytes(brem) + body
        for spec in [{}, {"subset_none": True}, {"key_prefix": b"a"}]:
            _relay(ctx, wire, spec, blob_remaining=brem)
        out, _ = _relay(ctx, wire, {}, blob_remaining=brem)
        assert out == changes
    blob = S.frame(bytes(5000), 2)
    out, _ = _relay(ctx, body + blob[:-10], {})
    assert out == changes
    cut = S.frame(S.change_payload(b"tail", 1, 2, 3, value=bytes(100)))
    g = ctx.decode_staged(body + cut[:-5])
    assert g["tail"] == 2
    out, _ = _relay(ctx, body + cut[:-5], {})
    assert out == changes
    # a batch that is all blob continuation: nothing to relay, and not an error
    ctx.decode_staged(bytes(100), blob_remaining=200)
    assert ctx.relay_staged(None) == (b"", 0)


def test_blob_skip_modes(ctx):
    """The same bytes with the batch staged whole and in blob-skipping pieces (whose earlier
    pieces stay on the device for the relay): the small C3-shaped stream, and one with 300 KB
    blobs that is long enough for the stage step to cut it into pieces that skip blob payload."""
    from _gpu import drp_amd
    small = S.c3_edge_stream(3)
    big = S.c3_stream(random.Random(9), 6, frames_per_unit=200, blob_len=300000) + S.c3_edge_stream(5)
    assert len(big) > 1 << 20
    try:
        for wire in [small, big]:
            for spec in [{}, {"change_range": (0, 50)}, {"key_prefix": b"00000007"}]:
                outs = []
                for mode in [drp_amd.BLOB_SKIP_OFF, drp_amd.BLOB_SKIP_ALWAYS]:
                    ctx.set_blob_skip(mode)
                    outs.append(_relay(ctx, wire, spec, decoded=False)[0])
                    if wire is big and mode == drp_amd.BLOB_SKIP_ALWAYS:
                        assert ctx.timing().h2d_skipped > 0  # (it was staged in pieces)
                assert outs[0] == outs[1]
        # the chunked form of the stage step, in pieces
        ctx.set_blob_skip(drp_amd.BLOB_SKIP_ALWAYS)
        want = _expected(big, {})[0]
        chunks = [big[i:i + 100003] for i in range(0, len(big), 100003)]
        ctx.decode_staged(chunks)
        assert ctx.relay_staged(None)[0] == want
        # the staged result stays valid after a relay: the rows fetched after it are the oracle's
        g = ctx.decode_staged(big)
        first = ctx.relay_staged(None)
        assert first[0] == want and ctx.relay_staged(None) == first
        ref = O.decode_batch(big)
        rows = ref["nframes"]
        assert g["nframes"] == rows
        o = drp_amd.alloc_host_outputs(rows)
        fr, co = drp_amd._structs(o, drp_amd._p)
        assert ctx.L.drp_decode_fetch(ctx.h, C.byref(fr), C.byref(co), 0, rows) == 0
        for k in ["payload_off", "payload_len", "type"]:
            np.testing.assert_array_equal(o[k], ref[k][:rows], err_msg=k)
        ch = (ref["type"][:rows] & 0x3F) == 1
        for k in O.COLS32 + O.COLS64 + ["flags"]:
            np.testing.assert_array_equal(o[k][ch], ref[k][:rows][ch], err_msg=k)
    finally:
        ctx.set_blob_skip(drp_amd.BLOB_SKIP_OFF)


@pytest.mark.parametrize("mode", ["off", "auto"])
def test_pinned_pipelined_batches(mode, monkeypatch):
    """A batch in page-locked memory on a ctx that pipelines in 1 MiB chunks (DRP_PIPE_CHUNK is
    read when the ctx opens): staged whole it is copied and decoded chunk by chunk; in AUTO mode a
    ctx's first batch probes in blob-skipping pieces and pipelines the rest, so the pipelined
    range starts past the batch's first staged byte. The relay's bytes are the oracle's."""
    import torch
    from _gpu import drp_amd
    wire = S.c3_stream(random.Random(13), 18, frames_per_unit=200, blob_len=300000)
    assert len(wire) > 5 << 20
    t = torch.empty(len(wire), dtype=torch.uint8, pin_memory=True)
    a = t.numpy()
    a[:] = np.frombuffer(wire, np.uint8)
    monkeypatch.setenv("DRP_PIPE_CHUNK", "1")
    with drp_amd.Ctx(0) as c:
        c.set_blob_skip(drp_amd.BLOB_SKIP_OFF if mode == "off" else drp_amd.BLOB_SKIP_AUTO)
        for spec in [{}, {"change_range": (0, 50)}, {"key_prefix": b"00000007"}]:
            want, idx, _, ref = _expected(wire, spec)
            for _ in range(2):  # (AUTO: the first batch probes, the later ones follow what it learned)
                g = c.decode_staged(a)
                assert g["nframes"] == ref["nframes"] == 18 * 201
                out, nsel = c.relay_staged(_filter(spec))
                assert nsel == len(idx) and out == want, (mode, spec)
    del t


def test_key_post_flags_do_not_leak(ctx, mixed):
    """With the key post-processing on (flags carry DRP_F_KEY_ASCII / _UTF8) the output is
    unchanged: the encoder rows' flags are masked to SUBSET | VALUE."""
    plain = _relay(ctx, mixed, {}, decoded=False)[0]
    assert _relay(ctx, mixed, {}, decoded=False, key_hash=True)[0] == plain
    assert _relay(ctx, mixed, {}, decoded=False, keys=True)[0] == plain
    g = ctx.decode_staged(mixed, keys=True)
    assert np.any(g["flags"] & 0x30)  # (the bits were there to leak)
    ctx.decode_staged(mixed)  # key post-processing off again


def test_idempotent(ctx, mixed):
    for spec in [{}, {"subset_none": True, "key_prefix": b"a"}]:
        out, _ = _relay(ctx, mixed, spec, decoded=False)
        again, idx = _relay(ctx, out, spec, decoded=False)
        assert again == out


# ---- error returns ---------------------------------------------------------------------------

def test_capacity(ctx, mixed):
    """cap one byte short: DRP_E_CAPACITY, *written = the size needed, nothing written (the guard
    bytes behind the buffer and the buffer itself stay as they were); host and device outputs."""
    import torch
    from _gpu import drp_amd
    want, idx, _, _ = _expected(mixed, {})
    ctx.decode_staged(mixed)
    need = len(want)
    buf = np.full(need + 64, 0xAB, np.uint8)
    with pytest.raises(drp_amd.DrpError) as e:
        ctx.relay_staged(None, cap=need - 1, out=buf)
    assert e.value.rc == drp_amd.DRP_E_CAPACITY and e.value.written == need
    assert np.all(buf == 0xAB)
    out, nsel = ctx.relay_staged(None, cap=need, out=buf)
    assert out == want and nsel == len(idx) and np.all(buf[need:] == 0xAB)
    # a device output buffer
    t = torch.full((need + 64,), 0xCD, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    written, ns = C.c_uint64(), C.c_uint64()
    rc = ctx.L.drp_relay_staged(ctx.h, None, C.c_void_p(t.data_ptr()), need - 1, C.byref(written), C.byref(ns))
    assert rc == drp_amd.DRP_E_CAPACITY and written.value == need
    assert bool(torch.all(t == 0xCD))
    rc = ctx.L.drp_relay_staged(ctx.h, None, C.c_void_p(t.data_ptr()), need, C.byref(written), C.byref(ns))
    assert rc == 0 and written.value == need and ns.value == len(idx)
    h = t.cpu().numpy()
    assert h[:need].tobytes() == want and np.all(h[need:] == 0xCD)


def test_invalid_arguments(ctx, mixed):
    from _gpu import drp_amd
    ctx.decode_staged(mixed)
    bad = [drp_amd.make_filter(flags=0x10), drp_amd.make_filter(change_range=(0, 1), flags=0x80000001),
           drp_amd.make_filter(subset=b"a", subset_none=True), drp_amd.make_filter(subset=bytes(257)),
           drp_amd.make_filter(key_prefix=bytes(257))]
    for f in bad:
        with pytest.raises(drp_amd.DrpError) as e:
            ctx.relay_staged(f)
        assert e.value.rc == drp_amd.DRP_E_INVAL
    assert ctx.relay_staged(drp_amd.make_filter(subset=bytes(256)))[1] == 0  # 256 bytes is allowed
    with drp_amd.Ctx(0) as fresh:  # nothing staged yet
        with pytest.raises(drp_amd.DrpError) as e:
            fresh.relay_staged(None)
        assert e.value.rc == drp_amd.DRP_E_INVAL


def test_host_encode_ends_the_staged_batch(ctx, mixed):
    """The staged wire shares the ctx's input staging with the encoder: after a host
    drp_encode_batch (a relay that also originates Changes) the relay refuses (DRP_E_INVAL)
    instead of reading overwritten or freed memory; the columns can still be fetched; a new stage
    relays again."""
    from _gpu import drp_amd
    want, idx, cols, ref = _expected(mixed, {})
    g = ctx.decode_staged(mixed)
    assert ctx.relay_staged(None)[0] == want
    big_heap = np.frombuffer(mixed * 3, np.uint8)  # (larger than the staged batch: the arena is reallocated)
    assert ctx.encode_batch(big_heap, cols) == want
    with pytest.raises(drp_amd.DrpError) as e:
        ctx.relay_staged(None)
    assert e.value.rc == drp_amd.DRP_E_INVAL
    rows = len(ref["type"])
    o = drp_amd.alloc_host_outputs(rows)
    fr, co = drp_amd._structs(o, drp_amd._p)
    assert ctx.L.drp_decode_fetch(ctx.h, C.byref(fr), C.byref(co), 0, rows) == 0
    np.testing.assert_array_equal(o["payload_off"], ref["payload_off"])
    ctx.decode_staged(mixed)
    assert ctx.relay_staged(None)[0] == want


def test_select_device_invalid_arguments(ctx):
    """drp_select_device's own argument checks and the filter checks it shares with the relay."""
    import torch
    from _gpu import drp_amd
    dev = torch.device("cuda", 0)
    n = 8
    wire_t = torch.zeros(64, dtype=torch.uint8, device=dev)
    cols = {"payload_off": torch.zeros(n, dtype=torch.int64, device=dev),
            "type": torch.zeros(n, dtype=torch.uint8, device=dev),
            "flags": torch.zeros(n, dtype=torch.uint8, device=dev)}
    for k in drp_amd.COLS32:
        cols[k] = torch.zeros(n, dtype=torch.int32, device=dev)
    for k in drp_amd.COLS64:
        cols[k] = torch.zeros(n, dtype=torch.int64, device=dev)
    rows = {k: torch.zeros(n, dtype=(torch.int32 if k.endswith("_len") else torch.uint8 if k == "flags"
                                     else torch.int64), device=dev) for k in SRC_KEYS}
    nsel_t = torch.full((1,), -1, dtype=torch.int64, device=dev)
    bad = [drp_amd.make_filter(flags=0x10), drp_amd.make_filter(subset=b"a", subset_none=True),
           drp_amd.make_filter(subset=bytes(257)), drp_amd.make_filter(key_prefix=bytes(257))]
    for f in bad:
        with pytest.raises(drp_amd.DrpError) as e:
            ctx.select_device(wire_t, cols, n, f, rows, None, nsel_t)
        assert e.value.rc == drp_amd.DRP_E_INVAL
    for miss in ["type", "change", "flags"]:  # a NULL input column
        with pytest.raises(drp_amd.DrpError) as e:
            ctx.select_device(wire_t, {**cols, miss: None}, n, None, rows, None, nsel_t)
        assert e.value.rc == drp_amd.DRP_E_INVAL
    with pytest.raises(drp_amd.DrpError) as e:  # a NULL output column
        ctx.select_device(wire_t, cols, n, None, {**rows, "key_off": None}, None, nsel_t)
    assert e.value.rc == drp_amd.DRP_E_INVAL
    with pytest.raises(drp_amd.DrpError) as e:  # no place for the count
        ctx.select_device(wire_t, cols, n, None, rows, None, None)
    assert e.value.rc == drp_amd.DRP_E_INVAL
    tp = lambda t: C.c_void_p(t.data_ptr())
    fr = drp_amd.Frames(tp(cols["payload_off"]), None, tp(cols["type"]))
    co = drp_amd.Changes(*[tp(cols[k]) for k in drp_amd.COLS32], tp(cols["change"]), tp(cols["from"]),
                         tp(cols["to"]), tp(cols["flags"]), None)
    dst = drp_amd.ChangeSrc(*[tp(rows[k]) for k in SRC_KEYS])
    # bytes NULL with nbytes > 0
    assert ctx.L.drp_select_device(ctx.h, None, 64, C.byref(fr), C.byref(co), n, None, C.byref(dst), None,
                                   tp(nsel_t)) == drp_amd.DRP_E_INVAL
    torch.cuda.synchronize()
    assert int(nsel_t.cpu()[0]) == -1  # nothing ran
    # and the valid call over the same (all-zero: no Change frame) columns selects nothing
    ctx.select_device(wire_t, cols, n, None, rows, None, nsel_t)
    torch.cuda.synchronize()
    assert int(nsel_t.cpu()[0]) == 0


# ---- drp_select_device -----------------------------------------------------------------------

def _device_select(ctx, streams, entry, spec, with_idx=True):
    """drp_decode_device over the streams laid end to end, then drp_select_device over its flat
    output. Returns the selected columns, sel_idx and the per-stream results."""
    import torch
    from _gpu import drp_amd
    dev = torch.device("cuda", 0)
    offs = np.concatenate([[0], np.cumsum([len(w) for w in streams])]).astype(np.int64)
    wire = np.frombuffer(b"".join(streams), np.uint8)
    wire_t = torch.from_numpy(wire.copy()).to(dev) if wire.size else torch.zeros(16, dtype=torch.uint8, device=dev)
    so_t, en_t = torch.from_numpy(offs).to(dev), torch.tensor(entry, dtype=torch.int64, device=dev)
    cap = int(wire.size) // 2 + 64
    outs = {"payload_off": torch.zeros(cap, dtype=torch.int64, device=dev),
            "payload_len": torch.zeros(cap, dtype=torch.int32, device=dev),
            "type": torch.zeros(cap, dtype=torch.uint8, device=dev),
            "flags": torch.zeros(cap, dtype=torch.uint8, device=dev)}
    for k in drp_amd.COLS32:
        outs[k] = torch.zeros(cap, dtype=torch.int32, device=dev)
    for k in drp_amd.COLS64:
        outs[k] = torch.zeros(cap, dtype=torch.int64, device=dev)
    rs = C.sizeof(drp_amd.StreamResult)
    res_t = torch.zeros(len(streams) * rs, dtype=torch.uint8, device=dev)
    ctx.decode_device(wire_t, so_t, en_t, outs, cap, res_t)
    raw = res_t.cpu().numpy().tobytes()
    res = [drp_amd.StreamResult.from_buffer_copy(raw[s * rs:(s + 1) * rs]) for s in range(len(streams))]
    n = sum(r.frames for r in res)
    rows = {k: torch.full((max(n, 1),), 0x55, dtype=(torch.int32 if k.endswith("_len") else
                                                     torch.uint8 if k == "flags" else torch.int64), device=dev)
            for k in SRC_KEYS}
    idx_t = torch.full((max(n, 1),), -1, dtype=torch.int64, device=dev) if with_idx else None
    nsel_t = torch.full((1,), -1, dtype=torch.int64, device=dev)
    ctx.select_device(wire_t, outs, n, _filter(spec), rows, idx_t, nsel_t)
    torch.cuda.synchronize()
    nsel = int(nsel_t.cpu()[0])
    got = {k: v.cpu().numpy() for k, v in rows.items()}
    return got, (idx_t.cpu().numpy() if with_idx else None), nsel, res, offs, wire, n


@pytest.mark.parametrize("spec", [{}, {"change_range": (0, 50)}, {"subset_none": True, "key_prefix": b"0"}])
def test_select_device_multi_stream(ctx, spec):
    """Three streams of unequal length in one drp_decode_device call, one of them empty and one
    entered behind a blob continuation: the selected columns and sel_idx equal the per-stream
    oracle's rows with the stream's offset added."""
    streams = [S.c2_stream(1500, seed=2).tobytes() + S.random_stream_seeded(11, 200), b"",
               S.random_stream_seeded(12, 90) + S.c2_stream(70, seed=5, start=40).tobytes()]
    pre = random.Random(4).randbytes(777)
    streams[2] = pre + streams[2]
    entry = [0, 0, len(pre)]
    got, sel_idx, nsel, res, offs, wire, n = _device_select(ctx, streams, entry, spec)
    want = {k: [] for k in SRC_KEYS}
    want_idx = []
    for s, w in enumerate(streams):
        ref = O.decode_batch(w[entry[s]:])
        assert res[s].frames == ref["nframes"]
        idx = np.flatnonzero(_mask(np.frombuffer(w[entry[s]:], np.uint8), ref, ref["nframes"], spec))
        cols = _rows(ref, idx, base=int(offs[s]) + entry[s])
        for k in SRC_KEYS:
            want[k].append(cols[k])
        want_idx.append(idx + res[s].frame_begin)
    want = {k: np.concatenate(v) for k, v in want.items()}
    want_idx = np.concatenate(want_idx)
    assert nsel == len(want_idx) and nsel > 0
    np.testing.assert_array_equal(sel_idx[:nsel].astype(np.uint64), want_idx.astype(np.uint64))
    for k in SRC_KEYS:
        np.testing.assert_array_equal(got[k][:nsel].astype(want[k].dtype), want[k], err_msg=k)
        assert np.all(got[k][nsel:] == (0x55 if k != "flags" else 0x55)), k  # nothing past the selection
    assert np.all(sel_idx[nsel:] == -1)
    # the rows encode, with the wire as the heap, to what the oracle encodes
    assert O.encode_changes(wire.tobytes(), {k: got[k][:nsel].astype(want[k].dtype) for k in SRC_KEYS}) == \
        O.encode_changes(wire.tobytes(), want)


@pytest.mark.parametrize("n", [0, 1, 64, 65, 1024, 1025])
def test_select_device_row_counts(ctx, n):
    """The compaction alone at the wave and workgroup edges, without sel_idx (NULL) and with."""
    wire = S.c2_stream(n, seed=6).tobytes()
    for spec in [{}, {"change_range": (0, 50)}, {"key_prefix": b"%010d" % max(n - 1, 0)}]:
        ref = O.decode_batch(wire)
        idx = np.flatnonzero(_mask(np.frombuffer(wire, np.uint8), ref, n, spec))
        want = _rows(ref, idx)
        for with_idx in [False, True]:
            got, sel_idx, nsel, res, _, _, rows = _device_select(ctx, [wire], [0], spec, with_idx)
            assert rows == n and nsel == len(idx)
            for k in SRC_KEYS:
                np.testing.assert_array_equal(got[k][:nsel].astype(want[k].dtype), want[k], err_msg=k)
            if with_idx:
                np.testing.assert_array_equal(sel_idx[:nsel], idx)
