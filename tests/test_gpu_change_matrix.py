"""GPU: every branch of the Change payload decode, on every kernel, at the places where the
decoders change readers. The payloads are tests/_change_model.py's matrix (one entry at least per
branch of the model, which tests/test_change_matrix.py holds against the oracle); each goes through
drp_decode_device as the odd frame of many small streams, placed by the tile arithmetic of
csrc/drp_spec.h (TILE 8192, HALO 512) and csrc/drp_decode.hip (TILE 4096 / 8192, HALO 512), and the
result is compared exactly with the oracle's decode of the stream and with the model's row."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import _change_model as M
import _oracle as O
import _streams as S

pytestmark = pytest.mark.gpu

HALO = 512
RES = np.dtype([(k, "<u8") for k in ["frame_begin", "frames", "changes", "blobs", "consumed", "blob_remaining",
                                     "err_frame"]] +
               [(k, "<u4") for k in ["err_code", "err_detail", "tail_kind", "reserved"]] + [("tail_frame_bytes", "<u8")])
C2 = S.c2_stream(400, seed=5).tobytes()  # canonical 86-byte Change frames
TRAIL = C2[86 * 397:]  # the three canonical frames behind the odd one
TINY = b"\x01\x02" * 6000  # empty blob frames, two bytes each
BLOB_BYTES = np.random.default_rng(1).integers(0, 256, 12100, dtype=np.uint8).tobytes()
FILL = bytes((7 * i + 3) & 0xFF for i in range(700))
COLS = O.COLS32 + O.COLS64 + ["flags"]


def _pad_frame(r):
    """A canonical Change frame of exactly r bytes (40 <= r < 126)."""
    f = S.frame(S.change_payload(b"pad", 1, 2, 3, value=bytes(range(r - 15))))
    assert len(f) == r
    return f


def _prefix(p):
    """Canonical frames, p bytes in all (0 or >= 40): (bytes, frames)."""
    if p == 0:
        return b"", 0
    n = (p - 40) // 86
    return C2[:86 * n] + _pad_frame(p - 86 * n), n + 1


def _behind_filler(payload, tile, inside):
    """`payload` behind an unknown bytes field sized so that, with the frame header 64 bytes before
    a tile edge, the 16-byte window of the payload's first field header (min(16, its length): what
    decode_change asks its reader for) ends exactly at TILE + HALO (inside the LDS image) or one
    byte past it (the reader reports ERR_UNREACHABLE and the decode starts over from the stream)."""
    need = min(16, len(payload))
    # a two-byte frame length, the id, the filler's tag and its two-byte length: six bytes
    f = 64 + HALO + (0 if inside else 1) - need - 6
    p = b"\x7a" + M.vi(f) + FILL[:f] + payload
    first = len(S.frame(p)) - len(payload)  # frame-relative offset of the payload's first header
    assert first + need == 64 + HALO + (0 if inside else 1)
    return p


def _streams_for(tile):
    """[(label, stream bytes, frames in its chain, index of the odd frame, odd payload)] for one
    tile size; the streams are laid end to end in this order, so a placement is an absolute
    position modulo the tile."""
    out, base = [], 0

    def put(label, payload, rel=None, trail=TRAIL, before=None, after=b"", n_before=0, n_after=0):
        nonlocal base
        fr = S.frame(payload)
        if before is None:  # a canonical prefix that puts frame offset `rel` on a tile edge
            p = (-(base + rel)) % tile
            if 0 < p < 40:
                p += tile
            before, n_before = _prefix(p)
            assert (base + len(before) + rel) % tile == 0
        w = before + fr + after + trail
        out.append((label, w, n_before + 1 + n_after + (3 if trail else 0), n_before, payload))
        base += len(w)

    entries = M.change_matrix()
    for e in entries:
        fr = S.frame(e.payload)
        hdr = len(fr) - len(e.payload)
        for j in (1, 2, 63, 0):  # the frame header starts j bytes before a tile edge
            put(f"{e.name}@hdr-{j}", e.payload, rel=j)
        # the tile edge inside the payload: in a tag, a length or a number where the entry marks
        # one, else behind its first byte and in its middle
        for k in (e.marks or (1, len(e.payload) // 2))[:2]:
            if k < len(e.payload):
                put(f"{e.name}@edge+{k}", e.payload, rel=hdr + k)
        put(f"{e.name}@img.inside", _behind_filler(e.payload, tile, True), rel=64)
        put(f"{e.name}@img.outside", _behind_filler(e.payload, tile, False), rel=64)
        put(f"{e.name}@stream.end", e.payload, rel=1, trail=b"")  # the payload ends the stream
    reach = M.reach_matrix(tile + HALO)
    for e in reach:
        for j in (1, 0, tile // 2):
            put(f"{e.name}@hdr-{j}", e.payload, rel=j)
    for e in entries + reach:
        # between canonical frames, in tiles that are not stream-edge tiles
        put(f"{e.name}@c2", e.payload, before=C2[:86 * 150], n_before=150, after=C2[86 * 150:86 * 300], n_after=150)
        put(f"{e.name}@dense", e.payload, before=TINY, n_before=6000, after=TINY, n_after=6000)
        # between blobs longer than a tile, the odd frame's header in the last byte of a thread's 64
        # (no other frame starts in that thread's bytes: emit_sparse wants one frame a thread at most)
        n = 12000 + (63 - (base + 12000 + 3)) % 64
        put(f"{e.name}@blobs", e.payload, before=S.frame(BLOB_BYTES[:n], 2), n_before=1,
            after=S.frame(BLOB_BYTES[100:], 2), n_after=1)
        assert (base - len(out[-1][1]) + n + 3) % 64 == 63
    return out


@functools.lru_cache(maxsize=None)
def _expected(tile):
    """The streams of one tile size with what they must decode to: the oracle's decode of every
    stream, the odd frame's row checked against the model here (so a kernel that equals this
    equals both)."""
    streams = _streams_for(tile)
    refs = []
    for label, w, chain, idx, payload in streams:
        r = O.decode_batch(w, cap=chain + 1)
        m = M.decode(payload)
        # an error stops the stream: the frames behind it are not delivered
        assert r["nframes"] == (idx if m["err"] else chain), label
        assert r["err_code"] == m["err"] and (not m["err"] or r["err_frame"] == idx), label
        assert len(r["type"]) > idx and r["type"][idx] == 1, label  # (the malformed row is kept)
        for k in COLS:
            assert int(r[k][idx]) == m[k] & (0xFFFFFFFF if k.endswith(("_off", "_len")) else ~0), (label, k)
        refs.append(r)
    return streams, refs


def _columns(dev, cap):
    import torch
    from _gpu import drp_amd
    outs = {"payload_off": torch.zeros(cap, dtype=torch.int64, device=dev),
            "payload_len": torch.zeros(cap, dtype=torch.int32, device=dev),
            "type": torch.zeros(cap, dtype=torch.uint8, device=dev),
            "flags": torch.zeros(cap, dtype=torch.uint8, device=dev)}
    for k in drp_amd.COLS32:
        outs[k] = torch.zeros(cap, dtype=torch.int32, device=dev)
    for k in drp_amd.COLS64:
        outs[k] = torch.zeros(cap, dtype=torch.int64, device=dev)
    return outs


def _check(streams, refs, res, host, rows_of, offs):
    """Per-stream results and the delivered rows (plus the malformed one) against the oracle."""
    labels = [s[0] for s in streams]

    def same(got, want, what):
        got, want = np.asarray(got), np.asarray(want)
        if not np.array_equal(got, want):
            i = int(np.flatnonzero(got != want)[0])
            s = i if len(got) == len(streams) else int(rows_of[i])
            raise AssertionError(f"{what}: {labels[s]} (stream {s}): got {got[i]}, want {want[i]}; "
                                 f"{int((got != want).sum())} of {len(got)} differ")

    ref = lambda k: np.array([r[k] for r in refs], np.uint64)
    same(res["frames"], ref("nframes"), "frames")
    same(res["changes"], ref("changes"), "changes")
    same(res["blobs"], ref("blobs"), "blobs")
    same(res["err_code"], ref("err_code"), "err_code")
    bad = ref("err_code") != 0
    same(np.where(bad, res["err_frame"], 0), np.where(bad, ref("err_frame"), 0), "err_frame")
    same(res["tail_kind"], ref("tail"), "tail")
    same(res["consumed"], ref("consumed"), "consumed")
    same(res["blob_remaining"], ref("blob_remaining"), "blob_remaining")
    cat = lambda k: np.concatenate([r[k] for r in refs])
    same(host["payload_off"].astype(np.int64) - offs[rows_of], cat("payload_off").astype(np.int64), "payload_off")
    same(host["payload_len"].astype(np.uint32), cat("payload_len"), "payload_len")
    same(host["type"], cat("type"), "type")
    ch = (cat("type") & 0x3F) == 1
    for k in COLS:
        want = cat(k)
        same(np.where(ch, host[k].astype(want.dtype), 0), np.where(ch, want, 0), k)


@pytest.mark.parametrize("kernel", ["speculative", "exact4096", "exact8192"])
def test_every_kind_every_kernel(kernel):
    """Every matrix entry at every placement and in every tile context, one drp_decode_device call
    per kernel; streams behind a failing stream are compared like any other. The placement streams
    are at most three tiles long; the context streams (@c2, @dense, @blobs) and the reach_matrix
    entries are longer on purpose (up to four tiles of 8192, seven of 4096), so that the odd frame's
    tile is an interior tile, or because the payload itself is longer than an LDS image.

    The speculative call must be decoded by the speculative kernels (drp_timing.strict_reruns == 0:
    no re-run of the call on the exact kernel) and the exact calls without a retry. Which emitter
    takes a tile is reported neither by drp_timing nor by the stats mode; the map below is read
    from the code. Exact kernel (decode_tiles), every placement and context: decode_change over
    LdsReader, and again over GlobalReader when a field header's window leaves TILE + HALO
    (@img.inside for the headers behind the first one, @img.outside, the reach_matrix entries).
    Speculative path, placements (@hdr-j, @edge+k, @stream.end: stream-edge tiles without per-frame
    records): emit_lean's in-place change_canon for the canonical entries, every other entry sends
    its tile to emit_tiles<false> (decode_change over LdsReader, then decode_change_hbm over
    GlobalReader for @img.* and the reach_matrix entries). @c2, interior tiles: entries in the
    records' shape stay in claims_fast's records (crec_frame) and emit_recs writes them; canonical
    ones outside that shape take emit_lean; the rest take emit_tiles<false>, which re-emits the
    canonical neighbours in the tile too. @dense: more than DRP_LCAP (1024) frames in the tile, so
    emit_tiles emits per thread (emit_frame) instead of from its LDS list. @blobs: the odd frame
    alone in its thread's 64 bytes of a tile with a handful of frames, emit_sparse decodes it from
    the stream through GlobalWinReader (change_canon_g for canonical entries, decode_change for the
    rest); so do the reach_matrix entries that start on a tile edge."""
    import torch

    from _gpu import drp_amd

    tile = 8192 if kernel == "speculative" else int(kernel[5:])
    streams, refs = _expected(tile)
    offs = np.concatenate([[0], np.cumsum([len(s[1]) for s in streams])]).astype(np.int64)
    wire = np.frombuffer(b"".join(s[1] for s in streams), np.uint8)
    assert wire.size < 96 << 20
    cap = sum(s[2] for s in streams) + 64  # (every frame of a chain takes a row, delivered or not)
    dev = torch.device("cuda", 0)
    wire_t = torch.from_numpy(wire.copy()).to(dev)
    so_t = torch.from_numpy(offs).to(dev)
    outs = _columns(dev, cap)
    assert C.sizeof(drp_amd.StreamResult) == RES.itemsize
    res_t = torch.zeros(len(streams) * RES.itemsize, dtype=torch.uint8, device=dev)
    with drp_amd.Ctx(0, tile=tile) as ctx:
        if kernel != "speculative":
            ctx.set_exact(True)
        ctx.decode_device(wire_t, so_t, None, outs, cap, res_t)
        tm = ctx.timing()
    # the kernels under test made the result: no fall-back of the speculative call to the exact
    # kernel, no second run of the exact one
    assert (tm.strict_reruns, tm.exact_retries) == (0, 0), (kernel, tm.strict_reruns, tm.exact_retries, tm.spec_repairs)
    res = res_t.cpu().numpy().view(RES)
    keep = np.array([len(r["type"]) for r in refs], np.int64)  # delivered rows + the malformed one
    rows_of = np.repeat(np.arange(len(streams)), keep)
    first = np.cumsum(keep) - keep
    idx = res["frame_begin"].astype(np.int64)[rows_of] + (np.arange(keep.sum()) - first[rows_of])
    assert idx.max() < cap
    idx_t = torch.from_numpy(idx).to(dev)
    host = {k: v[idx_t].cpu().numpy() for k, v in outs.items()}
    _check(streams, refs, res, host, rows_of, offs)


# ---- the malformed row ---------------------------------------------------------------------------

ERROR_CLASSES = ["num.cut1", "lone.tag.key", "num.eleven", "len.ge2p64", "tag.2p53", "key.len.2p53",
                 "value.len.past1", "unknown.bytes.past", "unknown.wire3", "unknown.wire7", "fixed32.cut2",
                 "fixed64.cut5", "missing.key", "missing.to", "empty"]


@pytest.fixture(scope="module")
def ctx():
    from _gpu import drp_amd
    c = drp_amd.Ctx(0)
    yield c
    c.set_blob_skip(drp_amd.BLOB_SKIP_AUTO)
    c.close()


def test_malformed_row_is_staged_and_not_relayed(ctx):
    """One payload of each error class behind 20 canonical frames: decode_staged gives row n_frames
    with the model's (= the oracle's) columns and DRP_F_BAD (DRP_F_MISSING with it for a missing
    required field), and relay_staged emits the 20 frames before it and nothing else."""
    by = {e.name: e for e in M.change_matrix()}
    good = C2[:86 * 20]
    for name in ERROR_CLASSES:
        p = by[name].payload
        m = M.decode(p)
        assert m["err"], name
        w = good + S.frame(p) + TRAIL
        g = ctx.decode_staged(w)
        assert ctx.timing().strict_reruns == 0, name  # (the speculative kernels decoded it)
        r = O.decode_batch(w)
        assert (g["nframes"], g["err_code"], g["err_frame"]) == (20, m["err"], 20) == \
            (r["nframes"], r["err_code"], r["err_frame"]), name
        assert g["type"].size == 21 and g["type"][20] == 1, name
        assert int(g["payload_off"][20]) == len(good) + len(S.frame(p)) - len(p) and int(g["payload_len"][20]) == len(p)
        for k in COLS:
            assert int(g[k][20]) == int(r[k][20]) == m[k] & (0xFFFFFFFF if k.endswith(("_off", "_len")) else ~0), (name, k)
        want = M.F_BAD | (M.F_MISSING if m["err"] == M.ERR_REQUIRED else 0)
        assert int(g["flags"][20]) & (M.F_BAD | M.F_MISSING) == want, name
        out, nsel = ctx.relay_staged()
        assert nsel == 20 and out == good, name


def test_capacity_edge_of_the_missing_field_code(ctx):
    """finalize_kernel reads flags[err row] to tell DRP_ERR_REQUIRED from DRP_ERR_CHANGE, and rows
    at or past the capacity are never written. Settled from the code and pinned here: no emitter
    records a payload error for a row it does not write, and a chain with a frame at index >= cap
    has more than cap frames, which sets the capacity bit. So no caller sees DRP_ERR_CHANGE for a
    missing field, with or without DRP_E_CAPACITY.
    drp_decode_device (the caller's cap is the kernels' cap): with the malformed frame at index
    >= cap the call returns DRP_E_CAPACITY and the stream's result reports no payload error; with
    the frame inside cap it reports DRP_ERR_REQUIRED, and DRP_OK once cap holds the whole chain.
    drp_decode_batch into host columns decodes into rows of the ctx's own and returns DRP_E_CAPACITY
    when frames + the malformed row exceed cap, the code being DRP_ERR_REQUIRED either way.
    drp_decode_stage sizes its rows from a guess (stage_cap in csrc/drp_api.hip: bytes / 32 + 1024
    on a fresh ctx) and decodes again when the chain is longer: the sweep runs over the frame
    counts around the one at which the missing-field frame's index equals that guess, and checks
    that it does straddle it."""
    import torch

    from _gpu import drp_amd
    missing = S.frame(M.fields(to=None))
    n = 50
    w = np.frombuffer(C2[:86 * n] + missing + TRAIL, np.uint8)
    dev = torch.device("cuda", 0)
    wire_t = torch.from_numpy(w.copy()).to(dev)
    so_t = torch.tensor([0, w.size], dtype=torch.int64, device=dev)
    for cap in (n - 1, n, n + 1, n + 3, n + 4, n + 5):
        outs = _columns(dev, cap)
        res_t = torch.zeros(RES.itemsize, dtype=torch.uint8, device=dev)
        rc = drp_amd.DRP_OK
        try:
            ctx.decode_device(wire_t, so_t, None, outs, cap, res_t)
        except drp_amd.DrpError as e:
            rc = e.rc
        assert rc == (drp_amd.DRP_OK if cap >= n + 4 else drp_amd.DRP_E_CAPACITY), (cap, rc)
        r = res_t.cpu().numpy().view(RES)[0]
        if cap > n:  # the row was stored: the code is the missing field's
            assert (r["err_code"], r["err_frame"], r["frames"]) == (drp_amd.ERR_REQUIRED, n, n), (cap, r)
            assert int(outs["flags"][n]) & 0x0C == 0x0C
        else:  # the row was never stored: no code is made up from flags that are not there
            assert r["err_code"] == drp_amd.ERR_NONE, (cap, r)
    for cap in (n - 1, n, n + 1, n + 4):
        o = drp_amd.alloc_host_outputs(cap)
        fr, co = drp_amd._structs(o, drp_amd._p)
        carry = drp_amd.Carry(0, 0, 0, 0, 0)
        nf, ef, ec, ed = C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_uint32()
        rc = ctx.L.drp_decode_batch(ctx.h, drp_amd._p(w), w.size, C.byref(carry), C.byref(fr), C.byref(co), cap,
                                    C.byref(nf), C.byref(ef), C.byref(ec), C.byref(ed))
        assert rc == (drp_amd.DRP_OK if cap > n else drp_amd.DRP_E_CAPACITY), (cap, rc)
        assert (ec.value, ef.value, nf.value) == (drp_amd.ERR_REQUIRED, n, n), (cap, ec.value, ef.value, nf.value)
        if cap > n:
            assert o["flags"][n] & 0x0C == 0x0C
    guess = lambda nbytes: nbytes // 32 + 1024  # stage_cap(), csrc/drp_api.hip, for a ctx's first batch
    tail = len(missing + TRAIL)
    edge = next(n for n in range(1024, 4096) if guess(2 * n + tail) <= n)  # first n the guess cannot hold
    assert guess(2 * edge + tail) == edge  # the missing-field frame's index is the guessed capacity
    for n in range(edge - 8, edge + 9):
        wire = b"\x01\x02" * n + missing + TRAIL
        with drp_amd.Ctx(0) as c:
            g = c.decode_staged(wire)
        assert (g["nframes"], g["err_code"], g["err_frame"]) == (n, drp_amd.ERR_REQUIRED, n), (n, g["err_code"])
        assert g["flags"].size == n + 1 and g["flags"][n] & 0x0C == 0x0C, n


# ---- DRP_FETCH_F64 --------------------------------------------------------------------------------

F64_VALUES = [2**53 - 1, 2**53, 2**53 + 1, 2**53 + 3, 2**54 + 2, 2**54 + 6, 2**63, 2**63 + 1025, 2**64 - 1025,
              2**64 - 1]


def _f64_frames():
    v = F64_VALUES
    return b"".join(S.frame(S.change_payload(b"key%d" % i, v[i], v[(i + 1) % 10], v[(i + 2) % 10], value=b"v"))
                    for i in range(10))


def _f64_check(g, r, shift=0):
    assert g["err_code"] == 0 and g["nframes"] == r["nframes"]
    ch = (r["type"] & 0x3F) == 1
    assert ch.sum() >= 10
    for k in ["change", "from", "to"]:
        want = np.array([float(int(x)) for x in r[k][ch]])  # (Python's int -> float is correctly rounded)
        assert g[k].dtype == np.float64
        np.testing.assert_array_equal(g[k][ch], want, err_msg=k)
    want = np.array([float(int(x)) for x in r["payload_off"]])
    np.testing.assert_array_equal(g["payload_off"], want, err_msg="payload_off")
    assert sorted(set(int(x) for x in r["change"][ch])) == sorted(F64_VALUES)


def test_fetch_f64_rounds_as_a_host_cast(ctx):
    """DRP_FETCH_F64 over numbers around 2^53, 2^54, 2^63 and 2^64 (ties to even both ways, the
    last one rounding up to 2^64): one staged piece, blob-skipping pieces (the host shifts the
    payload_off doubles of each piece) and a carried blob as row 0."""
    from _gpu import drp_amd
    fr = _f64_frames()
    assert float(2**53 + 1) == 2.0**53 and float(2**53 + 3) == 2.0**53 + 4 and float(2**64 - 1) == 2.0**64
    _f64_check(ctx.decode_staged(fr, block=True, f64=True), O.decode_batch(fr))
    rng = random.Random(9)
    w = b"".join(fr + S.frame(rng.randbytes(1 << 20), 2) for _ in range(3)) + fr
    ctx.set_blob_skip(drp_amd.BLOB_SKIP_ALWAYS)
    try:
        g = ctx.decode_staged(w, block=True, f64=True)
        assert ctx.timing().h2d_skipped > 0
    finally:
        ctx.set_blob_skip(drp_amd.BLOB_SKIP_AUTO)
    _f64_check(g, O.decode_batch(w))
    w = bytes(5000) + fr
    g = ctx.decode_staged(w, blob_remaining=5000, block=True, f64=True)
    r = O.decode_batch(w, blob_remaining=5000)
    assert g["type"][0] == 0x42 and g["payload_off"][0] == 0.0
    _f64_check(g, r)
