"""GPU parity for the fan-out of latest per key: drp_fanout_latest_staged and
drp_fanout_latest_device give, for every filter f of up to 64, exactly what drp_latest_staged /
drp_latest_device give for filters[f] over the same rows. Every comparison is bit-exact, first
against the CPU side of test_gpu_latest (the oracle's decode, the predicate in numpy, a dict from
identity to the best (change, row), the oracle's encoding of the winners), then against
latest_staged(filters[f]) called K times on the same staged batch."""
import ctypes as C
import random

import numpy as np
import pytest

import _oracle as O
import _streams as S
from _relay import SRC_KEYS, U64MAX, make_filter as _filter, mask as _mask, rows as _rows, winners as _winners
from test_gpu_latest import _blob_stream, _expected, _pool_rows, _wire, _with_blobs
from test_gpu_relay_wire_bounds import N as WB_N, _abs, _cuts, _out, _want, decoded  # noqa: F401 (decoded: a fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from _gpu import drp_amd
    c = drp_amd.Ctx(0)
    c.set_blob_skip(drp_amd.BLOB_SKIP_OFF)
    yield c
    c.close()


def _want_all(wire, specs, blob_remaining=0):
    """Per filter: (bytes, winner rows, best) of the expected side."""
    ex = [_expected(wire, spec, blob_remaining) for spec in specs]
    return [(e[0], e[1], e[4]) for e in ex], ex[0][3]


def _fl(ctx, wire, specs, blob_remaining=0, stage=None, want=None, singles=True):
    """Stage `wire` (or the chunk list `stage` that spells it), run drp_fanout_latest_staged and
    compare every output with the expected side, then with drp_latest_staged of that filter."""
    if want is None:
        want, ref = _want_all(wire, specs, blob_remaining)
        g = ctx.decode_staged(stage if stage is not None else wire, blob_remaining=blob_remaining)
        assert g["nframes"] == ref["nframes"] and g["err_code"] == ref["err_code"]
    else:
        ctx.decode_staged(stage if stage is not None else wire, blob_remaining=blob_remaining)
    filters = [_filter(s) for s in specs]
    outs, nsel = ctx.fanout_latest_staged(filters)
    assert nsel == [len(w[1]) for w in want], (nsel, [len(w[1]) for w in want])
    for f, spec in enumerate(specs):
        assert outs[f] == want[f][0], (f, spec, len(outs[f]), len(want[f][0]))
    if singles:
        for f, spec in enumerate(specs):
            assert ctx.latest_staged(filters[f]) == (outs[f], nsel[f]), (f, spec)
    return outs, want


# ---- row counts ------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4095, 4096, 4097, 8193])
def test_row_counts(ctx, n):
    """0, 1 and the wave (64) and the fan-out's workgroup (4096) sizes, one row below, at and above,
    and three workgroups; keys from a pool of n // 4, changes from a range of 5."""
    rows = _pool_rows(n, max(1, n // 4), 5, seed=n, subsets=(None, None, b"s"))
    specs = [{}, {"change_range": (1, 3)}, {"subset": b"s"}]
    outs, want = _fl(ctx, _wire(rows), specs)
    if n >= 63:
        assert all(0 < len(w[1]) < n for w in want)
        by_key = {}
        for r, (k, sub, ch) in enumerate(rows):
            by_key.setdefault((k, sub, ch), []).append(r)
        assert any(len(v) > 1 for v in by_key.values())  # (ties were there to break)
        assert len({(k, sub) for k, sub, _ in rows}) < n  # (keys repeat)


# ---- filter counts and pass widths -----------------------------------------------------------

def _specs(K):
    base = [{}, {"change_range": (0, 9)}, {"subset": b"s"}, {"key_prefix": b"key-1"},
            {"subset_none": True, "change_range": (3, 12)}, {"change_range": (15, 2)},
            {"key_prefix": b"key-2", "subset": b"tt"}]
    more = [{"change_range": (f % 5, f % 20), **({"subset": b"s"} if f % 3 == 0 else {})} for f in range(7, 64)]
    return (base + more)[:K]


@pytest.fixture(scope="module")
def seven_hundred():
    wire = _wire(_pool_rows(700, 60, 20, seed=17, subsets=(None, b"s", b"tt")))
    return wire, _want_all(wire, _specs(64))[0]


@pytest.mark.parametrize("K,widths", [(1, [0]), (2, [0, 1]), (7, [1, 3, 0]), (64, [1, 64, 0])])
def test_filter_counts_and_pass_widths(ctx, seven_hundred, K, widths):
    """K filters in passes of every listed width (0: the default; 3 at K = 7: an uneven last
    pass): every setting gives the expected bytes."""
    wire, want = seven_hundred
    try:
        for k, t in enumerate(widths):
            ctx.set_fanout_latest_pass(t)
            _fl(ctx, wire, _specs(K), want=want[:K], singles=k == 0)
    finally:
        ctx.set_fanout_latest_pass(0)
    if K == 64:
        assert len({w[0] for w in want}) > 20 and any(len(w[1]) == 0 for w in want)


# ---- the reduction is per filter --------------------------------------------------------------

def test_snapshots_differ_per_filter(ctx):
    """One identity with the changes 3, 5, 5 and 9 among others: change <= 4 gives the 3, <= 5 the
    later 5, 6..8 nothing, >= 9 and {} the 9."""
    rows = _pool_rows(300, 30, 12, seed=21, subsets=(None, b"s"))
    at = {40: 3, 90: 5, 150: 5, 220: 9}
    for r, ch in at.items():
        rows[r] = (b"the-one", None, ch)
    specs = [{"change_range": (0, 4)}, {"change_range": (0, 5)}, {"change_range": (6, 8)},
             {"change_range": (9, U64MAX)}, {}]
    wire = _wire(rows)
    want, _ = _want_all(wire, specs)
    ident = (False, b"", b"the-one")
    assert [w[2].get(ident, (None, None))[1] for w in want] == [40, 150, None, 220, 220]
    # identities with three different winners across the filters: no reduction shared between filters passes
    assert sum(len({w[2][i][1] for w in want if i in w[2]}) >= 3 for i in want[4][2]) >= 2
    _fl(ctx, wire, specs, want=want)


def test_cleared_word(ctx):
    """Under change 1..10 an identity with only change 0 has no candidate (its rows equal the
    cleared state word and must not be picked), another with 0 and 1 gives its 1; under {} beside
    it the first identity's last row wins."""
    rows = _pool_rows(200, 20, 12, seed=22)
    for r in [5, 70, 130]:
        rows[r] = (b"zero", None, 0)
    for r, ch in [(6, 0), (71, 1), (131, 0)]:
        rows[r] = (b"mix", None, ch)
    specs = [{"change_range": (1, 10)}, {}]
    wire = _wire(rows)
    want, _ = _want_all(wire, specs)
    zero, mix = (False, b"", b"zero"), (False, b"", b"mix")
    assert zero not in want[0][2] and want[0][2][mix] == (1, 71)
    assert want[1][2][zero] == (0, 130) and want[1][2][mix] == (1, 71)
    _fl(ctx, wire, specs, want=want)
    _fl(ctx, wire, specs[::-1], want=want[::-1])


def test_identity_constant_conditions(ctx):
    """Filters on a subset, subset_none and key prefixes: identities that are a candidate for
    exactly one filter and for none, a filter that keeps nothing and one with min > max."""
    rows = _pool_rows(700, 60, 6, seed=23, subsets=(None, b"s", b"tt", b""))
    specs = [{"subset": b"s"}, {"subset_none": True}, {"key_prefix": b"key-1"},
             {"key_prefix": b"key-2", "subset": b"tt"}, {"key_prefix": b"nothing"}, {"change_range": (7, 3)}]
    wire = _wire(rows)
    want, _ = _want_all(wire, specs)
    every = _expected(wire, {})[4]
    times = {i: sum(i in w[2] for w in want) for i in every}
    assert 0 in times.values() and 1 in times.values() and 2 in times.values()
    assert len(want[4][1]) == 0 and len(want[5][1]) == 0 and all(len(w[1]) > 2 for w in want[:4])
    _fl(ctx, wire, specs, want=want)


def test_change_extremes(ctx):
    """0, 1, 2^63 and 2^64 - 1 within one group (unsigned compare) under {} and under a range that
    ends at 2^63."""
    rows = [(b"big", None, 2**63), (b"zero", None, 0), (b"big", None, U64MAX), (b"big", None, 1), (b"big", None, 0),
            (b"zero", None, 0), (b"mid", None, 2**63), (b"mid", None, 2**63 - 1), (b"big", None, 2**63)]
    specs = [{}, {"change_range": (1, 2**63)}]
    wire = _wire(rows)
    want, _ = _want_all(wire, specs)
    assert list(want[0][1]) == [2, 5, 6] and list(want[1][1]) == [6, 8]
    _fl(ctx, wire, specs, want=want)


def test_hash_mask(ctx):
    """test_gpu_latest.test_hash_mask's 300 rows over 40 identities with the row hash cut to 0, 1
    and 3 bits and whole, four filters: the bytes never change."""
    rng = random.Random(40)
    idents = [(b"key%02d" % (k // 2), None if k % 2 else b"x") for k in range(40)]
    rows = [(*idents[k], 0) for k in range(40)] + [(*rng.choice(idents), rng.randrange(6)) for _ in range(260)]
    wire = _wire(rows)
    specs = [{}, {"change_range": (0, 2)}, {"subset": b"x"}, {"key_prefix": b"key1", "change_range": (1, 4)}]
    want, _ = _want_all(wire, specs)
    assert len(want[0][2]) == 40
    try:
        for k, mask in enumerate([0, 1, 7, U64MAX]):
            ctx.set_latest_hash_mask(mask)
            _fl(ctx, wire, specs, want=want, singles=k == 0)
    finally:
        ctx.set_latest_hash_mask(U64MAX)


# ---- frames around the Changes ---------------------------------------------------------------

SPECS3 = [{}, {"change_range": (0, 2)}, {"key_prefix": b"key-3"}]


def test_blobs_and_batch_edges(ctx):
    """Blobs between the Changes; a batch that starts inside a blob."""
    body = _with_blobs(_pool_rows(500, 40, 5, seed=7, subsets=(None, b"s")))
    plain, _ = _fl(ctx, body, SPECS3)
    for brem in [1000, 5]:
        wire = random.Random(brem).randbytes(brem) + body
        assert _fl(ctx, wire, SPECS3, blob_remaining=brem)[0] == plain


def test_error_ends_the_rows(ctx):
    """A type >= 3 and a malformed Change mid-way: nothing at or after the error takes part."""
    a = _pool_rows(200, 20, 5, seed=8)
    b = [(k, sub, ch + 100) for k, sub, ch in _pool_rows(50, 20, 5, seed=9)]
    wa, wb = _wire(a), _wire(b)
    specs = [{}, {"change_range": (2, 200)}]
    head = [e[0] for e in _want_all(wa, specs)[0]]
    for mid, code in [(b"\x03\x07ab", 1), (S.frame(b"\x12\x05ab"), 4)]:
        wire = wa + mid + wb
        assert O.decode_batch(wire)["err_code"] == code
        assert _fl(ctx, wire, specs)[0] == head


def test_blob_skip_modes_and_chunks(ctx):
    """The same bytes with the 1 MiB blob stream staged whole, in blob-skipping pieces and as a
    list of chunks."""
    from _gpu import drp_amd
    big = _blob_stream()
    assert len(big) > 1 << 20
    chunks = [big[i:i + 100003] for i in range(0, len(big), 100003)]
    specs = [{}, {"change_range": (0, 4)}, {"key_prefix": b"key-1", "subset": b"s"}]
    want, _ = _want_all(big, specs)
    try:
        for mode in [drp_amd.BLOB_SKIP_OFF, drp_amd.BLOB_SKIP_ALWAYS]:
            ctx.set_blob_skip(mode)
            _fl(ctx, big, specs, want=want, singles=mode == drp_amd.BLOB_SKIP_ALWAYS)
            if mode == drp_amd.BLOB_SKIP_ALWAYS:
                assert ctx.timing().h2d_skipped > 0  # (it was staged in pieces)
            _fl(ctx, big, specs, want=want, stage=chunks, singles=False)
    finally:
        ctx.set_blob_skip(drp_amd.BLOB_SKIP_OFF)


# ---- drp_fanout_latest_device ----------------------------------------------------------------

@pytest.fixture(scope="module")
def three_streams(ctx):
    """The flat decode of test_gpu_latest.test_latest_device_multi_stream: three streams that share
    keys, their rows end to end (device columns, read only), and the oracle's rows likewise."""
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
    refs = [O.decode_batch(s) for s in streams]
    assert [r.frames for r in res] == [r["nframes"] for r in refs] and n == 700 + 90 + 1300 + 6
    ref = {k: np.concatenate([r[k][:r["nframes"]] for r in refs]) for k in ["type", "flags"] + O.COLS32 + O.COLS64}
    ref["payload_off"] = np.concatenate([r["payload_off"][:r["nframes"]] + np.uint64(offs[s])
                                         for s, r in enumerate(refs)])
    return wire, wire_t, outs, n, ref, res[2].frame_begin


DEV_SPECS = [{}, {"change_range": (0, 3)}, {"subset_none": True, "key_prefix": b"key-1"}, {"key_prefix": b"nothing"}]


def _device(ctx, wire_t, cols, n, specs, rows_cap, with_idx=True):
    import torch
    rows, idx_t = _out(rows_cap + 8)
    rb_t = torch.full((len(specs) + 1,), -1, dtype=torch.int64, device=wire_t.device)
    ctx.fanout_latest_device(wire_t, cols, n, [_filter(s) for s in specs], rows, rows_cap, idx_t if with_idx else None,
                             rb_t)
    torch.cuda.synchronize()
    return rows, idx_t.cpu().numpy(), rb_t.cpu().numpy()


def test_fanout_latest_device_multi_stream(ctx, three_streams):
    """row_base, sel_idx and the ten row columns per output against the expected side; sentinels
    intact past row_base[K]; one encode_device of all rows gives the expected bytes end to end;
    the later stream wins a cross-stream tie."""
    import torch
    wire, wire_t, cols, n, ref, begin3 = three_streams
    w = np.frombuffer(wire, np.uint8)
    wins = [_winners(w, ref, np.flatnonzero(_mask(w, ref, n, spec))) for spec in DEV_SPECS]
    want_rb = np.concatenate([[0], np.cumsum([len(i) for i, _ in wins])])
    total = int(want_rb[-1])
    assert all(len(i) > 0 for i, _ in wins[:3]) and len(wins[3][0]) == 0
    best = wins[0][1]
    assert best[(False, b"", b"tie")][1] >= begin3 and best[(True, b"s", b"tie2")][1] >= begin3
    rows, idx, rb = _device(ctx, wire_t, cols, n, DEV_SPECS, total)
    np.testing.assert_array_equal(rb, want_rb)
    assert np.all(idx[total:] == -1)
    want_bytes = b""
    for f, (want_idx, _) in enumerate(wins):
        a, b = int(rb[f]), int(rb[f + 1])
        np.testing.assert_array_equal(idx[a:b], want_idx, err_msg=str(f))
        want = _rows(ref, want_idx)
        want_bytes += O.encode_changes(wire, want)
        for k in SRC_KEYS:
            got = rows[k].cpu().numpy()
            np.testing.assert_array_equal(got[a:b].astype(want[k].dtype), want[k], err_msg=f"{f} {k}")
            assert np.all(got[total:] == 0x55), k
    foff_t = torch.zeros(total + 1, dtype=torch.int64, device=wire_t.device)
    out_t = torch.zeros(4 * len(wire), dtype=torch.uint8, device=wire_t.device)
    ctx.encode_device(rows, wire_t, total, foff_t, out_t, 4 * len(wire))
    torch.cuda.synchronize()
    assert out_t.cpu().numpy()[:int(foff_t.cpu()[total])].tobytes() == want_bytes
    # rows_cap one short: row_base is still true and nothing is written
    rows, idx, rb = _device(ctx, wire_t, cols, n, DEV_SPECS, total - 1)
    np.testing.assert_array_equal(rb, want_rb)
    assert np.all(idx == -1) and all(np.all(rows[k].cpu().numpy() == 0x55) for k in SRC_KEYS)
    # without sel_idx
    rows, idx, rb = _device(ctx, wire_t, cols, n, DEV_SPECS, total, with_idx=False)
    np.testing.assert_array_equal(rb, want_rb)
    np.testing.assert_array_equal(rows["change"].cpu().numpy()[:total],
                                  np.concatenate([ref["change"][i] for i, _ in wins]).astype(np.int64))


@pytest.mark.parametrize("name", ["inside", "exact", "zero"])
def test_wire_bounds(ctx, decoded, name):  # noqa: F811
    """The wire cut short as test_gpu_relay_wire_bounds cuts it: a candidate's whole key, and its
    subset where it has one, lie within the cut. Output f equals latest_device(filters[f]) and the
    expected side under that rule (the keys are distinct: every candidate wins)."""
    import torch
    wire_t, cols, ref = decoded
    cut = _cuts(ref)[name]
    ak, asub = _abs(ref, "key"), _abs(ref, "subset")
    odd = np.arange(WB_N) % 2 == 1
    inside = (ak + 7 <= cut) & (~odd | (asub + 2 <= cut))
    specs = [{"key_prefix": b"key"}, {"subset": b"ab"}, {"change_range": (1, 3)}, {}]
    want = []
    for spec in specs:
        keep = np.zeros(WB_N, bool)
        keep[_want(ref, spec, cut) if spec else np.arange(WB_N)] = True
        want.append(np.flatnonzero(keep & inside))
    assert [len(x) for x in want] == {"inside": [70, 35, 30, 70], "exact": [70, 35, 30, 70], "zero": [0] * 4}[name]
    total = sum(len(x) for x in want)
    rows, idx, rb = _device(ctx, wire_t[:cut], cols, WB_N, specs, total)
    np.testing.assert_array_equal(rb, np.concatenate([[0], np.cumsum([len(x) for x in want])]))
    for f, spec in enumerate(specs):
        a, b = int(rb[f]), int(rb[f + 1])
        np.testing.assert_array_equal(idx[a:b], want[f], err_msg=str(spec))
        one, one_idx = _out(WB_N)
        nsel_t = torch.full((1,), -1, dtype=torch.int64, device=wire_t.device)
        ctx.latest_device(wire_t[:cut], cols, WB_N, _filter(spec), one, one_idx, nsel_t)
        torch.cuda.synchronize()
        assert int(nsel_t.cpu()[0]) == b - a
        np.testing.assert_array_equal(one_idx.cpu().numpy()[:b - a], want[f])
        exp = _rows(ref, want[f])
        for k in SRC_KEYS:
            got = rows[k].cpu().numpy()[a:b]
            np.testing.assert_array_equal(got, one[k].cpu().numpy()[:b - a], err_msg=f"{spec} {k}")
            np.testing.assert_array_equal(got.astype(exp[k].dtype), exp[k], err_msg=f"{spec} {k}")


# ---- error returns, determinism --------------------------------------------------------------

@pytest.fixture(scope="module")
def mixed():
    wire = _with_blobs(_pool_rows(800, 70, 6, seed=12, subsets=(None, b"s", b"")))
    return wire, _want_all(wire, SPECS3)[0]


GUARD64 = 0x5555555555555555


def _raw(ctx, filters, K, buf, cap):
    off, ns = np.full(66, GUARD64, np.uint64), np.full(65, GUARD64, np.uint64)
    from _gpu import drp_amd
    rc = ctx.L.drp_fanout_latest_staged(ctx.h, filters, K, drp_amd._p(buf), cap, drp_amd._p(off), drp_amd._p(ns))
    return rc, off, ns


def test_capacity(ctx, mixed):
    """cap one byte short: DRP_E_CAPACITY, out_off[K] = the size needed, out keeps its fill."""
    from _gpu import drp_amd
    wire, want = mixed
    ctx.decode_staged(wire)
    filters = [_filter(s) for s in SPECS3]
    need = sum(len(w[0]) for w in want)
    buf = np.full(need + 64, 0xAB, np.uint8)
    with pytest.raises(drp_amd.DrpError) as e:
        ctx.fanout_latest_staged(filters, cap=need - 1, out=buf)
    assert e.value.rc == drp_amd.DRP_E_CAPACITY and e.value.written == need
    assert e.value.n_selected == [len(w[1]) for w in want] and np.all(buf == 0xAB)
    outs, nsel = ctx.fanout_latest_staged(filters, cap=need, out=buf)
    assert outs == [w[0] for w in want] and np.all(buf[need:] == 0xAB)


def test_invalid_arguments(ctx, mixed):
    """nfilters 0 and 65, a bad filter in the middle, nothing staged and a staged batch a host
    encode has ended: DRP_E_INVAL; drp_decode_fetch still works afterwards."""
    from _gpu import drp_amd
    wire, want = mixed
    ref = O.decode_batch(wire)
    ctx.decode_staged(wire)
    buf = np.full(4096, 0xAB, np.uint8)
    arr65 = drp_amd.filter_array([None] * 65)
    for K in [0, 65]:
        rc, off, ns = _raw(ctx, arr65, K, buf, 4096)
        assert rc == drp_amd.DRP_E_INVAL and np.all(off == GUARD64) and np.all(buf == 0xAB)
    for bad in [drp_amd.make_filter(flags=0x10), drp_amd.make_filter(subset=b"a", subset_none=True),
                drp_amd.make_filter(key_prefix=bytes(257))]:
        with pytest.raises(drp_amd.DrpError) as e:
            ctx.fanout_latest_staged([None, bad, None])
        assert e.value.rc == drp_amd.DRP_E_INVAL
    with drp_amd.Ctx(0) as fresh:  # nothing staged yet
        with pytest.raises(drp_amd.DrpError) as e:
            fresh.fanout_latest_staged([None])
        assert e.value.rc == drp_amd.DRP_E_INVAL
    filters = [_filter(s) for s in SPECS3]
    assert ctx.fanout_latest_staged(filters)[0] == [w[0] for w in want]
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
    cols = _expected(wire, {})[2]
    assert ctx.encode_batch(np.frombuffer(wire * 3, np.uint8), cols) == want[0][0]
    with pytest.raises(drp_amd.DrpError) as e:
        ctx.fanout_latest_staged(filters)
    assert e.value.rc == drp_amd.DRP_E_INVAL
    ctx.decode_staged(wire)
    assert ctx.fanout_latest_staged(filters)[0] == [w[0] for w in want]


def test_device_invalid_arguments(ctx, three_streams):
    """drp_fanout_latest_device: nfilters 0 and 65, a bad filter in the middle, a NULL row_base."""
    import torch
    from _gpu import drp_amd
    wire, wire_t, cols, n, ref, _ = three_streams
    rows, idx_t = _out(16)
    rb_t = torch.full((66,), -1, dtype=torch.int64, device=wire_t.device)
    for filters in [[], [None] * 65, [None, drp_amd.make_filter(flags=0x10), None]]:
        with pytest.raises(drp_amd.DrpError) as e:
            ctx.fanout_latest_device(wire_t, cols, n, filters, rows, 16, idx_t, rb_t)
        assert e.value.rc == drp_amd.DRP_E_INVAL
    with pytest.raises(drp_amd.DrpError) as e:
        ctx.fanout_latest_device(wire_t, cols, n, [None], rows, 16, idx_t, None)
    assert e.value.rc == drp_amd.DRP_E_INVAL
    torch.cuda.synchronize()
    assert np.all(rb_t.cpu().numpy() == -1) and np.all(idx_t.cpu().numpy() == -1)


def test_deterministic(ctx, mixed):
    """The same call twice, and again after a drp_fanout_staged and a drp_latest_staged in between
    (they share the scratch and the page-locked filter table): identical results."""
    wire, want = mixed
    ctx.decode_staged(wire)
    filters = [_filter(s) for s in SPECS3]
    first = ctx.fanout_latest_staged(filters)
    assert first == ([w[0] for w in want], [len(w[1]) for w in want])
    assert ctx.fanout_latest_staged(filters) == first
    fan = ctx.fanout_staged(filters[::-1])[:2]
    one = ctx.latest_staged(filters[1])
    assert one == (want[1][0], len(want[1][1]))
    assert ctx.fanout_latest_staged(filters) == first
    assert ctx.fanout_staged(filters[::-1])[:2] == fan


def test_existing_entry_points_unchanged(ctx, mixed):
    """latest_staged, fanout_staged and relay_staged before and after a fanout_latest_staged call:
    the CPU side's bytes."""
    wire, want = mixed
    w = np.frombuffer(wire, np.uint8)
    ref = O.decode_batch(wire)
    sel = [O.encode_changes(wire, _rows(ref, np.flatnonzero(_mask(w, ref, ref["nframes"], s)))) for s in SPECS3]
    assert sel[0] != want[0][0] and sel[1] != want[1][0]  # (the snapshot is smaller than the selection)
    ctx.decode_staged(wire)
    filters = [_filter(s) for s in SPECS3]
    for _ in range(2):
        for f in range(3):
            assert ctx.latest_staged(filters[f])[0] == want[f][0]
            assert ctx.relay_staged(filters[f])[0] == sel[f]
        assert ctx.fanout_staged(filters)[0] == sel
        assert ctx.fanout_latest_staged(filters)[0] == [x[0] for x in want]
