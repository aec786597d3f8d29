"""GPU parity for the relay fan-out: drp_fanout_device (up to 64 filters over one pass of the
decoded columns, the kept rows of the filters end to end) and drp_fanout_staged (the same over
the staged batch, one encode for every output, and the splice table that says where the blob
frames belong). The expected side is always the CPU oracle: decode the wire, apply each filter's
predicate in numpy, encode the kept rows; the blob positions follow from the same row lists."""
import ctypes as C
import random

import numpy as np
import pytest

import _oracle as O
import _streams as S
from _relay import SRC_KEYS, U64MAX, make_filter as _filter, mask as _mask, rows as _rows
from test_gpu_select import _crafted, _mixed_specs

pytestmark = pytest.mark.gpu

FAN_ROWS = 4096   # rows per workgroup of fan_count (drp_fanout.hip: 1024 lanes, four rows each)
FAN_SCAN = 1024   # counts per first-level block of its scan
GUARD64 = 0x5555555555555555


@pytest.fixture(scope="module")
def ctx():
    from _gpu import drp_amd
    c = drp_amd.Ctx(0)
    c.set_blob_skip(drp_amd.BLOB_SKIP_OFF)
    yield c
    c.close()


# ---- the expected side ---------------------------------------------------------------------

def _key(spec):
    return tuple(sorted((k, v) for k, v in spec.items()))


class Expect:
    """The oracle's decode of one wire, and per distinct filter the kept rows and their encoding
    (computed once per filter, shared by every output that uses it)."""

    def __init__(self, wire, blob_remaining=0, cap=None):
        self.wire = wire
        self.w = np.frombuffer(wire, np.uint8) if len(wire) else np.zeros(0, np.uint8)
        self.ref = O.decode_batch(wire, blob_remaining=blob_remaining, cap=cap)
        self.n = self.ref["nframes"]
        self._memo = {}

    def of(self, spec):
        k = _key(spec)
        if k not in self._memo:
            idx = np.flatnonzero(_mask(self.w, self.ref, self.n, spec))
            self._memo[k] = (idx, O.encode_changes(self.wire, _rows(self.ref, idx)))
        return self._memo[k]


def _fan(ctx, ex, specs, blob_remaining=0, splice=False, stage=True, **stage_kw):
    """Stage ex.wire (unless it is staged already), fan out, compare every output with the oracle."""
    if stage:
        g = ctx.decode_staged(ex.wire, blob_remaining=blob_remaining, **stage_kw)
        assert g["nframes"] == ex.n and g["err_code"] == ex.ref["err_code"]
    outs, nsel, sp = ctx.fanout_staged([_filter(s) for s in specs], splice=splice)
    assert len(outs) == len(nsel) == len(specs)
    for f, spec in enumerate(specs):
        idx, want = ex.of(spec)
        assert nsel[f] == len(idx), (f, spec, nsel[f], len(idx))
        assert outs[f] == want, (f, spec, len(outs[f]), len(want))
    return outs, nsel, sp


def _c2_specs(n):
    return [{}, {"change_range": (1000, 2000)}, {"change_range": (0, 50)}, {"key_prefix": b"%010d" % 0},
            {"key_prefix": b"%010d" % max(n - 1, 0)}]


# ---- row counts x K --------------------------------------------------------------------------

_c2_memo = {}


def _c2(n):
    if n not in _c2_memo:
        _c2_memo[n] = Expect(S.c2_stream(n, seed=3).tobytes(), cap=n + 8)
    return _c2_memo[n]


@pytest.mark.parametrize("K", [1, 2, 33, 64])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, FAN_ROWS - 1, FAN_ROWS, FAN_ROWS + 1])
def test_row_counts(ctx, n, K):
    """0, 1 and the wave (64), the select's workgroup (1024) and the fan-out's workgroup (4096 rows)
    sizes, one row below, at and above, with 1, 2, 33 and 64 filters: all rows, none, the half with
    change <= 50, only the first and only the last row, cycled so that neighbours differ. K = 1
    takes each of the five in turn and also equals drp_relay_staged with the same filter."""
    ex = _c2(n)
    five = _c2_specs(n)
    counts = [n, 0, sum(1 for i in range(n) if i % 100 < 50), min(n, 1), min(n, 1)]
    ctx.decode_staged(ex.wire)
    if K == 1:
        for spec, cnt in zip(five, counts):
            outs, nsel, _ = _fan(ctx, ex, [spec], stage=False)
            assert nsel == [cnt]
            assert (outs[0], nsel[0]) == ctx.relay_staged(_filter(spec))
        return
    specs = [five[(f + K) % 5] for f in range(K)]
    outs, nsel, _ = _fan(ctx, ex, specs, stage=False)
    assert nsel == [counts[(f + K) % 5] for f in range(K)]


def test_scan_past_one_block(ctx):
    """The flattened count table holds (K + 1) * ceil(n / 4096) counts (one plane per filter and one
    for the blob rows), scanned in first-level blocks of 1024. With K = 64 it passes one block when
    65 * ceil(n / 4096) > 1024, that is from 16 workgroups on: n = 15 * 4096 + 1, the smallest.
    Filters 0 and 63 keep everything, 31 nothing (an empty output in the middle), 10 and 11 are the
    same, 40 keeps only the very last row."""
    K = 64
    n = 15 * FAN_ROWS + 1
    assert (K + 1) * ((n + FAN_ROWS - 1) // FAN_ROWS) > FAN_SCAN >= (K + 1) * ((n - 1) // FAN_ROWS)
    ex = Expect(S.c2_stream(n, seed=4).tobytes(), cap=n + 8)
    assert ex.n == n
    all_, none, half, first, last = _c2_specs(n)
    cyc = [half, none, first, last, {"change_range": (10, 20)}]
    specs = [cyc[f % 5] for f in range(K)]
    specs[0] = specs[63] = all_
    specs[31] = none
    specs[10] = specs[11] = half
    specs[40] = last
    outs, nsel, _ = _fan(ctx, ex, specs)
    assert nsel[0] == nsel[63] == n and nsel[31] == 0 and nsel[40] == 1 and nsel[10] == nsel[11] > 0
    assert outs[10] == outs[11] and outs[31] == b""
    assert ex.of(last)[0][0] == n - 1


# ---- every condition, per-filter tables ------------------------------------------------------

@pytest.fixture(scope="module")
def mixed():
    wire = S.random_stream_seeded(5, 300) + _crafted() + S.random_stream_seeded(6, 300)
    return Expect(wire)


@pytest.mark.parametrize("L", [0, 1, 255, 256])
@pytest.mark.parametrize("K", [27, 64])
def test_mixed_content_every_condition(ctx, mixed, K, L):
    """Blobs, id-0 headers, crafted subsets and keys; the whole list of single-filter conditions of
    test_gpu_select as one fan-out, cut or padded (cycled) to K filters, with a subset and a key
    prefix of L bytes at filter index 0 and at index K - 1, in both arrangements, so the byte table is
    indexed at both ends."""
    base = _mixed_specs(mixed.wire)
    specs = [base[f % len(base)] for f in range(K)]
    sub = bytes(range(256))[:L]          # the crafted rows hold subsets b"", range(255) and range(256)
    pre = (b"x" * 300)[:L]               # and a key of 300 x
    hits = {0: 2, 255: 1, 256: 1}
    for a, b in [({"subset": sub}, {"key_prefix": pre}), ({"key_prefix": pre}, {"subset": sub})]:
        specs[0], specs[K - 1] = a, b
        _fan(ctx, mixed, specs)
    if L in hits:
        assert len(mixed.of({"subset": sub})[0]) >= hits[L]
    assert len(mixed.of({"key_prefix": pre})[0]) >= 1


def test_overlapping_and_disjoint_filters(ctx, mixed):
    """A row matched by many filters appears in each of them; disjoint filters partition the rows."""
    ch = mixed.ref["change"][:mixed.n][(mixed.ref["type"][:mixed.n] & 0x3F) == 1]
    v = int(np.sort(ch)[len(ch) // 2])
    parts = [{"change_range": (0, v - 1)}, {"change_range": (v, v)}, {"change_range": (v + 1, U64MAX)}]
    specs = [{}] * 7 + parts + [{"key_prefix": b""}] * 3
    outs, nsel, _ = _fan(ctx, mixed, specs)
    every = mixed.of({})[0]
    assert all(k == len(every) for k in nsel[:7] + nsel[10:]) and len(set(outs[:7] + outs[10:])) == 1
    got = np.sort(np.concatenate([mixed.of(s)[0] for s in parts]))
    np.testing.assert_array_equal(got, every)  # (the oracle's three lists partition the Changes)
    assert sum(nsel[7:10]) == len(every) and min(nsel[7:10]) > 0


# ---- drp_fanout_device -----------------------------------------------------------------------

def _device_fanout(ctx, streams, entry, specs, short=0, with_idx=True, blob_cap=None):
    """drp_decode_device over the streams laid end to end, then drp_fanout_device over its flat
    output, against the per-stream oracle. short: rows_cap that much below the true total."""
    import torch
    from _gpu import drp_amd
    dev = torch.device("cuda", 0)
    K = len(specs)
    offs = np.concatenate([[0], np.cumsum([len(w) for w in streams])]).astype(np.int64)
    wire = np.frombuffer(b"".join(streams), np.uint8)
    wire_t = torch.from_numpy(wire.copy()).to(dev) if wire.size else torch.zeros(16, dtype=torch.uint8, device=dev)
    so_t, en_t = torch.from_numpy(offs).to(dev), torch.tensor(entry, dtype=torch.int64, device=dev)
    cap = int(wire.size) // 2 + 64
    cols = {"payload_off": torch.zeros(cap, dtype=torch.int64, device=dev),
            "payload_len": torch.zeros(cap, dtype=torch.int32, device=dev),
            "type": torch.zeros(cap, dtype=torch.uint8, device=dev),
            "flags": torch.zeros(cap, dtype=torch.uint8, device=dev)}
    for k in drp_amd.COLS32:
        cols[k] = torch.zeros(cap, dtype=torch.int32, device=dev)
    for k in drp_amd.COLS64:
        cols[k] = torch.zeros(cap, dtype=torch.int64, device=dev)
    rs = C.sizeof(drp_amd.StreamResult)
    res_t = torch.zeros(len(streams) * rs, dtype=torch.uint8, device=dev)
    ctx.decode_device(wire_t, so_t, en_t, cols, cap, res_t)
    raw = res_t.cpu().numpy().tobytes()
    res = [drp_amd.StreamResult.from_buffer_copy(raw[s * rs:(s + 1) * rs]) for s in range(len(streams))]
    n = sum(r.frames for r in res)
    # the oracle, stream by stream
    want = [{k: [] for k in SRC_KEYS} for _ in specs]
    want_idx = [[] for _ in specs]
    blobs = []
    for s, w in enumerate(streams):
        ref = O.decode_batch(w[entry[s]:])
        assert res[s].frames == ref["nframes"]
        wv = np.frombuffer(w[entry[s]:], np.uint8)
        blobs.append(np.flatnonzero((ref["type"][:ref["nframes"]] & 0x3F) == 2) + res[s].frame_begin)
        for f, spec in enumerate(specs):
            idx = np.flatnonzero(_mask(wv, ref, ref["nframes"], spec))
            rows = _rows(ref, idx, base=int(offs[s]) + entry[s])
            for k in SRC_KEYS:
                want[f][k].append(rows[k])
            want_idx[f].append(idx + res[s].frame_begin)
    want = [{k: np.concatenate(v) for k, v in d.items()} for d in want]
    want_idx = [np.concatenate(v).astype(np.int64) for v in want_idx]
    blobs = np.concatenate(blobs).astype(np.int64)
    base = np.concatenate([[0], np.cumsum([len(v) for v in want_idx])]).astype(np.int64)
    total = int(base[-1])
    rows_cap = total - short
    room = total + 70  # (the arrays are longer than rows_cap: the guard behind it is checked too)
    rows = {k: torch.full((room,), 0x55, dtype=(torch.int32 if k.endswith("_len") else
                                                torch.uint8 if k == "flags" else torch.int64), device=dev)
            for k in SRC_KEYS}
    idx_t = torch.full((room,), -1, dtype=torch.int64, device=dev) if with_idx else None
    rb_t = torch.full((K + 1,), -1, dtype=torch.int64, device=dev)
    sp = None
    if blob_cap is not None:
        sp = {"blob_row": torch.full((blob_cap,), GUARD64, dtype=torch.int64, device=dev),
              "blob_rank": torch.full((max(K * blob_cap, 1),), GUARD64, dtype=torch.int64, device=dev),
              "n_blobs": torch.full((1,), -1, dtype=torch.int64, device=dev)}
    ctx.fanout_device(wire_t, cols, n, [_filter(s) for s in specs], rows, rows_cap, idx_t, rb_t, sp)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(rb_t.cpu().numpy(), base)  # the true counts, whatever rows_cap is
    got = {k: v.cpu().numpy() for k, v in rows.items()}
    sel_idx = idx_t.cpu().numpy() if with_idx else None
    kept = total if short <= 0 else 0  # rows_cap too small: nothing is written
    for f in range(K if kept else 0):
        a, b = int(base[f]), int(base[f + 1])
        for k in SRC_KEYS:
            np.testing.assert_array_equal(got[k][a:b].astype(want[f][k].dtype), want[f][k], err_msg=f"{f} {k}")
        if with_idx:
            np.testing.assert_array_equal(sel_idx[a:b], want_idx[f], err_msg=str(f))
    for k in SRC_KEYS:
        assert np.all(got[k][kept:] == 0x55), k  # (every element was filled with the value 0x55)
    if with_idx:
        assert np.all(sel_idx[kept:] == -1)
    if sp is not None:
        assert int(sp["n_blobs"].cpu()[0]) == len(blobs)
        brow, brank = sp["blob_row"].cpu().numpy(), sp["blob_rank"].cpu().numpy()
        if len(blobs) <= blob_cap:
            np.testing.assert_array_equal(brow[:len(blobs)], blobs)
            assert np.all(brow[len(blobs):] == GUARD64)
            for f in range(K):
                np.testing.assert_array_equal(brank[f * blob_cap:f * blob_cap + len(blobs)],
                                              np.searchsorted(want_idx[f], blobs), err_msg=str(f))
        else:
            assert np.all(brow == GUARD64) and np.all(brank == GUARD64)
    return total, len(blobs)


def _three_streams():
    streams = [S.c2_stream(1500, seed=2).tobytes() + S.random_stream_seeded(11, 200), b"",
               S.random_stream_seeded(12, 90) + S.c2_stream(70, seed=5, start=40).tobytes()]
    pre = random.Random(4).randbytes(777)
    streams[2] = pre + streams[2]
    return streams, [0, 0, len(pre)]


_DEV_SPECS = [{}, {"change_range": (0, 50)}, {"subset_none": True, "key_prefix": b"0"}, {"change_range": (7, 3)},
              {"key_prefix": b"0000000042"}, {}]


def test_fanout_device_multi_stream(ctx):
    """Three streams of unequal length in one drp_decode_device call, one of them empty and one
    entered behind a blob continuation: out_rows, sel_idx and row_base equal the per-stream oracle's
    rows with the stream's offset added, nothing is written past row_base[K] (guard 0x55), and the
    device splice table lists the blob rows and, per filter, the kept rows before each."""
    streams, entry = _three_streams()
    total, nblobs = _device_fanout(ctx, streams, entry, _DEV_SPECS, blob_cap=64)
    assert total > 0 and 0 < nblobs <= 64
    _device_fanout(ctx, streams, entry, _DEV_SPECS[:1], with_idx=False)  # sel_idx NULL, no splice
    _device_fanout(ctx, streams, entry, _DEV_SPECS, blob_cap=nblobs - 1)  # the blob arrays stay untouched
    _device_fanout(ctx, [b"", b""], [0, 0], _DEV_SPECS, blob_cap=4)  # no rows at all


def test_rows_cap_overflow(ctx):
    """rows_cap one below the true total: row_base is correct, every out_rows and sel_idx entry
    still holds the guard pattern."""
    streams, entry = _three_streams()
    total, _ = _device_fanout(ctx, streams, entry, _DEV_SPECS, short=1)
    assert total > 1


# ---- errors, batch edges, modes --------------------------------------------------------------

_EDGE_SPECS = [{}, {"key_prefix": b""}, {"change_range": (0, 2**40)}, {"subset_none": True}, {"key_prefix": b"a"}]


@pytest.mark.parametrize("bad", ["type", "change", "required"])
def test_error_in_the_stream(ctx, bad):
    """An error mid-way (a type >= 3, a malformed Change, a Change without its key): nothing at or
    after the error frame appears in any output."""
    a, b = S.random_stream_seeded(7, 120), S.random_stream_seeded(8, 50)
    mid = {"type": b"\x03\x07ab", "change": S.frame(b"\x12\x05ab"),
           "required": S.frame(b"\x18\x01\x20\x02\x28\x03")}[bad]
    ex, exa = Expect(a + mid + b), Expect(a)
    assert ex.ref["err_code"] == {"type": 1, "change": 4, "required": 5}[bad] and ex.n == exa.n
    outs, _, _ = _fan(ctx, ex, _EDGE_SPECS)
    assert outs == [exa.of(s)[1] for s in _EDGE_SPECS]


def test_batch_edges(ctx):
    """A batch that starts inside a blob (blob_remaining 5 and 1000), one that ends in a partial
    blob, one that ends inside a Change, and one that is all blob continuation (every output empty,
    not an error)."""
    body = S.random_stream_seeded(9, 200)
    changes = [Expect(body).of(s)[1] for s in _EDGE_SPECS]
    for brem in [1000, 5]:
        wire = random.Random(brem).randbytes(brem) + body
        outs, _, _ = _fan(ctx, Expect(wire, blob_remaining=brem), _EDGE_SPECS, blob_remaining=brem)
        assert outs == changes
    blob = S.frame(bytes(5000), 2)
    outs, _, _ = _fan(ctx, Expect(body + blob[:-10]), _EDGE_SPECS)
    assert outs == changes
    cut = S.frame(S.change_payload(b"tail", 1, 2, 3, value=bytes(100)))
    ex = Expect(body + cut[:-5])
    assert ex.ref["tail"] == 2
    outs, _, _ = _fan(ctx, ex, _EDGE_SPECS)
    assert outs == changes
    ctx.decode_staged(bytes(100), blob_remaining=200)
    outs, nsel, sp = ctx.fanout_staged([None, _filter({"change_range": (0, 5)})], splice=True)
    assert outs == [b"", b""] and nsel == [0, 0] and sp["n_blobs"] == 0


def test_blob_skip_modes(ctx):
    """The batch staged whole and in blob-skipping pieces (300 KB blobs, long enough to be cut into
    pieces that skip blob payload): the outputs and the splice table are identical."""
    from _gpu import drp_amd
    big = S.c3_stream(random.Random(9), 6, frames_per_unit=200, blob_len=300000) + S.c3_edge_stream(5)
    ex = Expect(big)
    specs = [{}, {"change_range": (0, 50)}, {"key_prefix": b"00000007"}, {"change_range": (60, 70)}]
    res = []
    try:
        for mode in [drp_amd.BLOB_SKIP_OFF, drp_amd.BLOB_SKIP_ALWAYS]:
            ctx.set_blob_skip(mode)
            outs, nsel, sp = _fan(ctx, ex, specs, splice=True)
            if mode == drp_amd.BLOB_SKIP_ALWAYS:
                assert ctx.timing().h2d_skipped > 0  # (it was staged in pieces)
            res.append((outs, nsel, sp["n_blobs"], sp["blob_row"].tolist(), sp["blob_pos"].tolist()))
    finally:
        ctx.set_blob_skip(drp_amd.BLOB_SKIP_OFF)
    assert res[0] == res[1] and res[0][2] == 7
    _check_splice(ex, specs, ctx.decode_staged(big), *ctx.fanout_staged([_filter(s) for s in specs], splice=True))


# ---- the splice table --------------------------------------------------------------------------

def _blob_frame(wire, g, row):
    """Header, id and the payload bytes the batch holds of the blob at fetch row `row`."""
    po, pl = int(g["payload_off"][row]), int(g["payload_len"][row])
    return S.varint(pl + 1) + b"\x02" + bytes(wire[po:po + pl])


def _check_splice(ex, specs, g, outs, nsel, sp, nf0=0):
    """Inserting every blob's frame at blob_pos into output f gives the input with the unkept
    Changes removed and the kept ones canonical: byte for byte the oracle's frames in stream order,
    and, decoded again by the oracle, the kept rows' types and columns row for row."""
    ref, n = ex.ref, ex.n
    blob_rows = np.flatnonzero(((ref["type"][:n] & 0x3F) == 2) & ((ref["type"][:n] & 0x40) == 0))
    assert sp["n_blobs"] == len(blob_rows)
    np.testing.assert_array_equal(sp["blob_row"], blob_rows)  # (the oracle numbers rows as the fetch does)
    assert np.all((g["type"][sp["blob_row"].astype(np.int64)] & 0x3F) == 2)
    for f, spec in enumerate(specs):
        idx = ex.of(spec)[0]
        pos = sp["blob_pos"][f]
        assert np.all(np.diff(pos.astype(np.int64)) >= 0) and (len(pos) == 0 or int(pos[-1]) <= len(outs[f]))
        rec, at = [], 0
        for j, row in enumerate(sp["blob_row"]):
            rec.append(outs[f][at:int(pos[j])])
            rec.append(_blob_frame(ex.wire, g, int(row)))
            at = int(pos[j])
        rec.append(outs[f][at:])
        rec = b"".join(rec)
        order = np.sort(np.concatenate([idx, blob_rows]))  # the rows that survive, in stream order
        want = b"".join(_blob_frame(ex.wire, ref, r) if (ref["type"][r] & 0x3F) == 2 else
                        O.encode_changes(ex.wire, _rows(ref, np.array([r]))) for r in order)
        assert rec == want, (f, spec)
        d = O.decode_batch(rec)
        assert d["nframes"] == len(order) and d["err_code"] == 0
        np.testing.assert_array_equal(d["type"][:len(order)] & 0x3F, ref["type"][order] & 0x3F)
        isch = (ref["type"][order] & 0x3F) == 1
        for k in ["change", "from", "to", "key_len", "subset_len", "value_len"]:
            np.testing.assert_array_equal(d[k][:len(order)][isch], ref[k][order][isch], err_msg=k)
        np.testing.assert_array_equal(d["flags"][:len(order)][isch] & 3, ref["flags"][order][isch] & 3)
        np.testing.assert_array_equal(d["payload_len"][:len(order)][~isch], ref["payload_len"][order][~isch])


def _splice_stream():
    """Blob first; two blobs in a row; a blob between two Changes of which a filter keeps only the
    later one; a blob as the last whole frame; a final partial blob."""
    ch = lambda k, c, **kw: S.frame(S.change_payload(k, c, 1, 2, **kw))
    blob = lambda n, seed: S.frame(random.Random(seed).randbytes(n), 2)
    parts = [blob(300, 1), ch(b"a", 5, value=b"v"), ch(b"b", 6), blob(0, 2), blob(70, 3), ch(b"c", 7, subset=b"s"),
             ch(b"early", 10), blob(200, 4), ch(b"late", 20, value=b"xyz"), ch(b"d", 8), blob(33, 5),
             blob(500, 6)[:-100]]
    return b"".join(parts)


_SPLICE_SPECS = [{}, {"change_range": (20, 20)}, {"change_range": (1000, 2000)}, {"change_range": (0, 7)},
                 {"key_prefix": b"late"}, {"subset": b"s"}]


def test_splice_table(ctx):
    """The crafted stream of _splice_stream under six filters: inserting each blob's frame at blob_pos
    reproduces the input with the unkept Changes removed and the kept ones canonical."""
    wire = _splice_stream()
    ex = Expect(wire)
    assert ex.ref["tail"] == 3 and ex.n == 12
    g = ctx.decode_staged(wire)
    outs, nsel, sp = _fan(ctx, ex, _SPLICE_SPECS, splice=True, stage=False)
    assert sp["n_blobs"] == 6 and sp["blob_row"].tolist() == [0, 3, 4, 7, 10, 11]
    _check_splice(ex, _SPLICE_SPECS, g, outs, nsel, sp)
    # the filter that keeps only "late": the blob between "early" and "late" goes before its only Change
    assert nsel[1] == 1 and sp["blob_pos"][1].tolist() == [0, 0, 0, 0, len(outs[1]), len(outs[1])]
    # with the filter that keeps all, the spliced stream is the oracle's re-encoding of the whole input
    assert sp["blob_pos"][0][0] == 0 and sp["blob_pos"][0][-1] == len(outs[0])


def test_splice_after_a_leading_continuation(ctx):
    """blob_row is in fetch-row numbering (row 0 is the continuation, which is not listed)."""
    brem = 7
    wire = bytes(range(brem)) + _splice_stream()
    ex = Expect(wire, blob_remaining=brem)
    g = ctx.decode_staged(wire, blob_remaining=brem)
    assert g["type"][0] == 0x42
    outs, nsel, sp = _fan(ctx, ex, _SPLICE_SPECS, splice=True, stage=False)
    assert sp["blob_row"].tolist() == [1, 4, 5, 8, 11, 12]
    _check_splice(ex, _SPLICE_SPECS, g, outs, nsel, sp)


def test_splice_blob_cap_too_small(ctx):
    """blob_cap one below the true count: n_blobs is the true count, the arrays keep their guard
    pattern, and the outputs are still right."""
    ex = Expect(_splice_stream())
    ctx.decode_staged(ex.wire)
    outs, nsel, sp = ctx.fanout_staged([_filter(s) for s in _SPLICE_SPECS], splice=True, blob_cap=5)
    assert sp["n_blobs"] == 6 and sp["blob_row"] is None and sp["blob_pos"] is None
    assert all(np.all(a == GUARD64) for a in sp["raw"])
    assert outs == [ex.of(s)[1] for s in _SPLICE_SPECS]
    _, _, sp = ctx.fanout_staged([_filter(s) for s in _SPLICE_SPECS], splice=True, blob_cap=6)
    assert sp["blob_row"].tolist() == [0, 3, 4, 7, 10, 11]


# ---- capacity and arguments ----------------------------------------------------------------

def _raw_staged(ctx, filters, out_ptr, cap):
    from _gpu import drp_amd
    K = len(filters)
    off, ns = np.full(K + 1, GUARD64, np.uint64), np.full(max(K, 1), GUARD64, np.uint64)
    rc = ctx.L.drp_fanout_staged(ctx.h, drp_amd.filter_array(filters), K, out_ptr, cap, drp_amd._p(off),
                                 drp_amd._p(ns), None, None, 0, None)
    return rc, off, ns


def test_capacity(ctx, mixed):
    """cap one byte short: DRP_E_CAPACITY, out_off[K] = the size needed, n_selected valid, nothing
    written (the buffer and the guard bytes behind it stay as they were); host and device outputs."""
    import torch
    from _gpu import drp_amd
    specs = [{}, {"subset_none": True}, {"key_prefix": b"key"}]
    want = [mixed.of(s)[1] for s in specs]
    need = sum(len(w) for w in want)
    ctx.decode_staged(mixed.wire)
    flt = [_filter(s) for s in specs]
    buf = np.full(need + 64, 0xAB, np.uint8)
    with pytest.raises(drp_amd.DrpError) as e:
        ctx.fanout_staged(flt, cap=need - 1, out=buf)
    assert e.value.rc == drp_amd.DRP_E_CAPACITY and e.value.written == need
    assert e.value.n_selected == [len(mixed.of(s)[0]) for s in specs]
    assert np.all(buf == 0xAB)
    outs, nsel, _ = ctx.fanout_staged(flt, cap=need, out=buf)
    assert outs == want and np.all(buf[need:] == 0xAB)
    t = torch.full((need + 64,), 0xCD, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    rc, off, ns = _raw_staged(ctx, flt, C.c_void_p(t.data_ptr()), need - 1)
    assert rc == drp_amd.DRP_E_CAPACITY and int(off[3]) == need and ns.tolist() == nsel
    assert bool(torch.all(t == 0xCD))
    rc, off, ns = _raw_staged(ctx, flt, C.c_void_p(t.data_ptr()), need)
    assert rc == 0 and off.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    h = t.cpu().numpy()
    assert h[:need].tobytes() == b"".join(want) and np.all(h[need:] == 0xCD)


def test_invalid_arguments(ctx, mixed):
    """nfilters 0 and 65, one bad filter at index K - 1 (nothing runs: the outputs keep their guard),
    no staged batch."""
    from _gpu import drp_amd
    ctx.decode_staged(mixed.wire)
    buf = np.full(len(mixed.wire) * 4, 0xAB, np.uint8)
    for K in [0, 65]:
        rc, off, ns = _raw_staged(ctx, [None] * K, drp_amd._p(buf), buf.size)
        assert rc == drp_amd.DRP_E_INVAL and np.all(off == GUARD64)
    bad = [drp_amd.make_filter(flags=0x10), drp_amd.make_filter(subset=b"a", subset_none=True),
           drp_amd.make_filter(subset=bytes(257)), drp_amd.make_filter(key_prefix=bytes(257))]
    for b in bad:
        rc, off, ns = _raw_staged(ctx, [None, _filter({"subset": b"abc"}), None, b], drp_amd._p(buf), buf.size)
        assert rc == drp_amd.DRP_E_INVAL and np.all(off == GUARD64) and np.all(ns == GUARD64) and np.all(buf == 0xAB)
    outs, nsel, _ = ctx.fanout_staged([drp_amd.make_filter(subset=bytes(256)), None])  # 256 bytes is allowed
    assert nsel[0] == 0 and outs[1] == mixed.of({})[1]
    with drp_amd.Ctx(0) as fresh:  # nothing staged yet
        with pytest.raises(drp_amd.DrpError) as e:
            fresh.fanout_staged([None])
        assert e.value.rc == drp_amd.DRP_E_INVAL


def test_fanout_device_invalid_arguments(ctx):
    """drp_fanout_device: nfilters 0 and 65, a bad filter at the last index, NULL pointers; nothing
    runs (row_base keeps its guard), and the valid call over the same all-zero columns selects nothing."""
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
    rb_t = torch.full((66,), -1, dtype=torch.int64, device=dev)
    calls = [dict(filters=[]), dict(filters=[None] * 65), dict(filters=[None, drp_amd.make_filter(flags=0x10)]),
             dict(filters=[None, drp_amd.make_filter(key_prefix=bytes(257))]),
             dict(filters=[None], cols={**cols, "change": None}), dict(filters=[None], rows={**rows, "key_off": None}),
             dict(filters=[None], rb=None)]
    for kw in calls:
        with pytest.raises(drp_amd.DrpError) as e:
            ctx.fanout_device(wire_t, kw.get("cols", cols), n, kw["filters"], kw.get("rows", rows), n, None,
                              kw.get("rb", rb_t))
        assert e.value.rc == drp_amd.DRP_E_INVAL
    torch.cuda.synchronize()
    assert bool(torch.all(rb_t == -1))
    ctx.fanout_device(wire_t, cols, n, [None, None], rows, n, None, rb_t)
    torch.cuda.synchronize()
    assert rb_t.cpu().tolist()[:3] == [0, 0, 0]


def test_host_encode_ends_the_staged_batch(ctx, mixed):
    """After a host drp_encode_batch the fan-out refuses (DRP_E_INVAL), as the relay does; a new
    stage works again."""
    from _gpu import drp_amd
    idx, want = mixed.of({})
    ctx.decode_staged(mixed.wire)
    assert ctx.fanout_staged([None])[0] == [want]
    assert ctx.encode_batch(np.frombuffer(mixed.wire * 3, np.uint8), _rows(mixed.ref, idx)) == want
    with pytest.raises(drp_amd.DrpError) as e:
        ctx.fanout_staged([None])
    assert e.value.rc == drp_amd.DRP_E_INVAL
    ctx.decode_staged(mixed.wire)
    assert ctx.fanout_staged([None, None])[0] == [want, want]


def test_key_post_flags_do_not_leak(ctx, mixed):
    """With the key post-processing on (flags carry DRP_F_KEY_ASCII / _UTF8) the bytes are the same."""
    specs = [{}, {"key_prefix": b"key"}, {"subset_none": True}]
    plain, _, _ = _fan(ctx, mixed, specs)
    assert _fan(ctx, mixed, specs, keys=True)[0] == plain
    g = ctx.decode_staged(mixed.wire, keys=True)
    assert np.any(g["flags"] & 0x30)  # (the bits were there to leak)
    ctx.decode_staged(mixed.wire)  # key post-processing off again
