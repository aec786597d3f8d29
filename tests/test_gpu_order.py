"""GPU parity for the ordered catch-up (drp_order_device, Store.catch_up): the encoder rows of every
segment of a fan-out's output in ascending `change` (unsigned 64-bit, ties by input position), cut to
a per-segment limit, the outputs end to end. Every comparison is exact. The expected side is numpy:
np.argsort(change.astype(np.uint64), kind="stable") per segment, then the cut; wires are compared with
the oracle's encoding of the rows in that order."""
import collections

import numpy as np
import pytest

import _oracle as O
import _streams as S
from _relay import SRC_KEYS as SRC, U64MAX, change_at, down as _down, dtype as _dtype, up as _up

pytestmark = pytest.mark.gpu

GUARD = 0x5A
TILE, SCAN = 4096, 1024  # the sort workgroup's pairs and the counts of one first-level scan block


@pytest.fixture(scope="module")
def ctx():
    from _gpu import drp_amd
    assert (drp_amd.ORDER_TILE, drp_amd.ORDER_SCAN) == (TILE, SCAN)
    c = drp_amd.Ctx(0)
    yield c
    c.close()


# ---- inputs, the call, the expected side ---------------------------------------------------------

def _rows(change, cap=None):
    """Encoder rows with the given change column; every other column is a different function of the
    row index, so a row that lands in the wrong place shows in each of them. cap: the arrays' entries."""
    change = np.asarray(change, np.uint64)
    n = len(change)
    cap = n if cap is None else cap
    i = np.arange(cap, dtype=np.uint64)
    cols = {"key_off": i * 7 + 1, "key_len": i * 3 + 2, "subset_off": (i << 33) + 3, "subset_len": i % 97,
            "value_off": i * 13 + 5, "value_len": (i * 5) % 1001, "change": np.zeros(cap, np.uint64),
            "from": i ^ 0x5555, "to": i * 2 + 9, "flags": i % 4}
    cols["change"][:n] = change
    return {k: v.astype(_dtype(k)) for k, v in cols.items()}


def _guards(cap, K):
    """The guard pattern (every byte GUARD) for out_rows, out_sel_idx and out_base."""
    full = lambda n, dt: np.full(n * np.dtype(dt).itemsize, GUARD, np.uint8).view(dt)
    return {k: full(max(cap, 1), _dtype(k)) for k in SRC}, full(max(cap, 1), np.uint64), full(K + 1, np.uint64)


def _call(ctx, rows, base, limit=None, keep_ties=False, cap=None, sel=True, c=None):
    """drp_order_device over rows (numpy columns) and base (row_base); every output array starts as
    a guard pattern. Returns (out_rows, out_sel_idx, out_base) as numpy arrays, whole."""
    c = c or ctx
    K = len(base) - 1
    cap = len(rows["change"]) if cap is None else cap
    g_rows, g_sel, g_base = _guards(cap, K)
    d_rows = {k: _up(v if len(v) else np.zeros(1, v.dtype)) for k, v in rows.items()}
    d_out = {k: _up(v) for k, v in g_rows.items()}
    d_sel = _up(np.arange(max(cap, 1), dtype=np.uint64)) if sel else None
    d_osel = _up(g_sel) if sel else None
    d_base, d_obase = _up(np.asarray(base, np.uint64)), _up(g_base)
    c.order_device(d_rows, d_base, K, cap, d_out, d_obase, limit=limit, keep_ties=keep_ties, sel_idx_t=d_sel,
                   out_sel_idx_t=d_osel)
    return {k: _down(v) for k, v in d_out.items()}, _down(d_osel) if sel else None, _down(d_obase)


def _expect(change, base, limit=None, keep_ties=False):
    """(the source row of every output row, out_base): per segment the stable argsort, then the cut."""
    change = np.asarray(change, np.uint64)
    K = len(base) - 1
    lim = [limit] * K if limit is None or isinstance(limit, int) else list(limit)
    perm, ob = [], [0]
    for f in range(K):
        lo, hi = int(base[f]), int(base[f + 1])
        order = lo + np.argsort(change[lo:hi].astype(np.uint64), kind="stable")
        cnt = hi - lo
        kept = cnt if lim[f] is None else min(cnt, lim[f])
        if keep_ties and 0 < kept < cnt:
            while kept < cnt and change[order[kept]] == change[order[kept - 1]]:
                kept += 1
        perm.append(order[:kept])
        ob.append(ob[-1] + kept)
    return (np.concatenate(perm) if perm else np.zeros(0, np.int64)).astype(np.int64), np.array(ob, np.uint64)


def _check(ctx, change, base=None, limit=None, keep_ties=False, cap=None, c=None):
    """One call against the expected side: out_base entry by entry, every column of every kept row,
    sel_idx, and the guard pattern at and beyond out_base[nseg]. Returns (perm, out_base)."""
    change = np.asarray(change, np.uint64)
    base = [0, len(change)] if base is None else base
    rows = _rows(change, cap)
    out, osel, obase = _call(ctx, rows, base, limit, keep_ties, cap, c=c)
    perm, want_base = _expect(change, base, limit, keep_ties)
    np.testing.assert_array_equal(obase, want_base)
    total = int(want_base[-1])
    assert total == len(perm)
    np.testing.assert_array_equal(osel[:total], perm.astype(np.uint64))
    g_rows, g_sel, _ = _guards(len(osel), len(base) - 1)
    np.testing.assert_array_equal(osel[total:], g_sel[total:])
    for k in SRC:
        np.testing.assert_array_equal(out[k][:total], rows[k][perm], err_msg=k)
        np.testing.assert_array_equal(out[k][total:], g_rows[k][total:], err_msg=k + " (guard)")
    return perm, want_base


def _uniform(n, seed):
    return np.random.default_rng(seed).integers(0, 2**64, size=n, dtype=np.uint64)


# ---- row counts and tile edges ---------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1])
def test_row_counts(ctx, n):
    """One segment of n rows, keys uniform in [0, 2^64): 0, 1, the wave and the sort workgroup's tile,
    one below, at and one above; the arrays hold five entries more than the rows."""
    _check(ctx, _uniform(n, n), cap=n + 5)


def test_scan_past_one_block(ctx):
    """A pass's count table holds 256 * ceil(n / TILE) counts, scanned in first-level blocks of SCAN:
    it passes one block from five workgroups on, n = 4 * TILE + 1 the smallest."""
    n = 4 * TILE + 1
    assert 256 * ((n + TILE - 1) // TILE) > SCAN >= 256 * ((n - 1) // TILE)
    _check(ctx, _uniform(n, 7))
    _check(ctx, _uniform(n, 8), base=[0, 5, TILE + 3, TILE + 3, 3 * TILE, n])


# ---- digit positions -------------------------------------------------------------------------------

def _digit_cases():
    n = 3000
    rng = np.random.default_rng(3)
    byte = lambda: rng.integers(0, 256, size=n, dtype=np.uint64)
    fixed = np.uint64(0x1122334455667788)
    pick = np.array([2**63 - 1, 2**63, 2**64 - 1, 0], np.uint64)
    srt = np.sort(_uniform(n, 5))
    return {
        "byte7": (fixed & np.uint64(0x00FFFFFFFFFFFFFF)) | (byte() << np.uint64(56)),
        "byte0": (fixed & np.uint64(0xFFFFFFFFFFFFFF00)) | byte(),
        "bytes34": (fixed & np.uint64(0xFFFFFF0000FFFFFF)) | (byte() << np.uint64(24)) | (byte() << np.uint64(32)),
        "equal": np.full(n, fixed, np.uint64),
        "sign": pick[rng.integers(0, 4, size=n)],
        "sorted": srt,
        "reverse": srt[::-1].copy(),
    }


@pytest.mark.parametrize("case", ["byte7", "byte0", "bytes34", "equal", "sign", "sorted", "reverse"])
@pytest.mark.parametrize("K", [1, 3])
def test_digit_positions(ctx, case, K):
    """Keys that differ only in byte 7, only in byte 0, only in bytes 3 and 4, not at all, keys around
    2^63 (a signed compare would put 2^63 and 2^64 - 1 first), keys sorted already and in reverse; as
    one segment and as three."""
    change = _digit_cases()[case]
    perm, _ = _check(ctx, change, base=[0, len(change)] if K == 1 else [0, 1000, 1001, len(change)])
    if case == "sign" and K == 1:
        got = change[perm]
        assert got[0] == 0 and got[-1] == np.uint64(2**64 - 1) and np.all(got[:-1] <= got[1:])


def test_every_pass_runs(ctx, monkeypatch):
    """With constant-digit passes left on (DRP_ORDER_SKIP=0, read when a ctx opens) the same small keys
    go through all eight digit passes and the segment pass: the same result."""
    from _gpu import drp_amd
    monkeypatch.setenv("DRP_ORDER_SKIP", "0")
    c = drp_amd.Ctx(0)
    try:
        change = np.random.default_rng(9).integers(0, 100, size=5000, dtype=np.uint64)
        _check(ctx, change, base=[0, 700, 700, 4100, 5000], c=c)
        _check(ctx, change, c=c)
    finally:
        c.close()


# ---- stability -------------------------------------------------------------------------------------

def test_stable(ctx):
    """5,000 rows with change = i % 3 and sel_idx = arange: within each run of equal change
    out_sel_idx increases, and every output column equals the input's at out_sel_idx."""
    n = 5000
    change = (np.arange(n) % 3).astype(np.uint64)
    rows = _rows(change)
    out, osel, obase = _call(ctx, rows, [0, n])
    assert list(obase) == [0, n]
    got = out["change"][:n]
    assert np.all(got[:-1] <= got[1:])
    same = got[:-1] == got[1:]
    assert np.all(osel[1:n][same] > osel[:n - 1][same])
    assert sorted(osel[:n]) == list(range(n))
    for k in SRC:
        np.testing.assert_array_equal(out[k][:n], rows[k][osel[:n].astype(np.int64)], err_msg=k)


# ---- segments --------------------------------------------------------------------------------------

def _lengths(K):
    """Segment lengths for K segments: empty ones (the first, the last, two adjacent), 1, 64, lengths
    that straddle the tile, and odd ones that put boundaries inside a wave."""
    mix = [0, 1, 64, TILE + 1, 0, 0, 37, TILE - 1, 100, 1, 0, 63, 65, 2 * TILE + 5, 3]
    if K == 1:
        return [TILE + 77]
    if K == 2:
        return [TILE - 30, 95]
    ln = [mix[f % len(mix)] for f in range(K)]
    ln[-1] = 0
    return ln


@pytest.mark.parametrize("K", [1, 2, 33, 64])
@pytest.mark.parametrize("keys", ["few", "uniform"])
def test_segments(ctx, K, keys):
    """K segments of mixed lengths; with keys from {0 .. 4} the same keys stand on both sides of every
    boundary, and no row may cross it (the expected side sorts every segment on its own)."""
    ln = _lengths(K)
    base = np.concatenate([[0], np.cumsum(ln)]).astype(np.uint64)
    n = int(base[-1])
    if K > 2:
        assert ln[0] == 0 and ln[-1] == 0 and any(a == 0 and b == 0 for a, b in zip(ln, ln[1:]))
        assert any(int(b) % 64 for b in base[1:-1])
    change = (np.random.default_rng(K).integers(0, 5, size=n, dtype=np.uint64) if keys == "few" else _uniform(n, K))
    perm, ob = _check(ctx, change, base=list(base), cap=n + 3)
    np.testing.assert_array_equal(ob, base)
    for f in range(K):
        seg = perm[int(base[f]):int(base[f + 1])]
        assert np.all((seg >= int(base[f])) & (seg < int(base[f + 1])))


def test_row_base_not_from_zero(ctx):
    """row_base[0] > 0: the rows before it belong to no segment and reach no output."""
    change = np.random.default_rng(2).integers(0, 1000, size=700, dtype=np.uint64)
    perm, ob = _check(ctx, change, base=[130, 400, 400, 700])
    assert list(ob) == [0, 270, 270, 570] and perm.min() == 130


# ---- limit -----------------------------------------------------------------------------------------

def test_limits(ctx):
    """Per-segment limits 0, 1, cnt - 1, cnt, cnt + 1 and UINT64_MAX, exact and with KEEP_TIES, over
    uniform keys (no ties: both cut alike) and over keys with long runs; a NULL limit equals all
    UINT64_MAX. out_base is checked entry by entry and the outputs are contiguous (_check)."""
    cnt = [300, 300, 300, 300, 300, 300, TILE + 9]
    base = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
    n = int(base[-1])
    lim = [0, 1, 299, 300, 301, U64MAX, 1000]
    for change in [_uniform(n, 21), np.random.default_rng(22).integers(0, 7, size=n, dtype=np.uint64)]:
        for keep in [False, True]:
            _, ob = _check(ctx, change, base=list(base), limit=lim, keep_ties=keep)
            if not keep:
                assert list(np.diff(ob.astype(np.int64))) == [0, 1, 299, 300, 300, 300, 1000]
    a = _check(ctx, change, base=list(base), limit=None)
    b = _check(ctx, change, base=list(base), limit=[U64MAX] * len(cnt))
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])


def test_cut_inside_ties(ctx):
    """change = [1] * 10 + [2] * 20 + [3] * 10 in shuffled positions, limit 15 (inside the run of
    2s): without the flag exactly 15 rows, the first by position; with it the whole run, 30. A run that
    reaches the segment's end keeps cnt rows (limit 35 -> 40). With the flag and limit 0: 0 rows."""
    change = np.array([1] * 10 + [2] * 20 + [3] * 10, np.uint64)
    change = change[np.random.default_rng(4).permutation(40)]
    two = np.flatnonzero(change == 2)
    perm, ob = _check(ctx, change, limit=15, keep_ties=False)
    assert list(ob) == [0, 15] and list(perm[10:]) == list(two[:5])
    perm, ob = _check(ctx, change, limit=15, keep_ties=True)
    assert list(ob) == [0, 30] and list(perm[10:]) == list(two)
    assert list(_check(ctx, change, limit=35, keep_ties=True)[1]) == [0, 40]
    assert list(_check(ctx, change, limit=30, keep_ties=True)[1]) == [0, 30]  # (the cut at a run's end stays)
    assert list(_check(ctx, change, limit=0, keep_ties=True)[1]) == [0, 0]
    # a long run across several tiles, the cut in its middle
    big = np.concatenate([np.zeros(100, np.uint64), np.full(3 * TILE, 5, np.uint64), np.full(50, 9, np.uint64)])
    assert list(_check(ctx, big, limit=TILE, keep_ties=True)[1]) == [0, 100 + 3 * TILE]
    assert list(_check(ctx, big, limit=TILE, keep_ties=False)[1]) == [0, TILE]


# ---- untouched memory and capacity -------------------------------------------------------------------

@pytest.mark.parametrize("base", ["past_cap", "decreasing"])
def test_invalid_row_base(ctx, base):
    """row_base[nseg] = rows_cap + 1, and a row_base that decreases: out_base is all 0 and nothing
    else is written."""
    n = 500
    rows = _rows(_uniform(n, 1))
    rb = [0, 200, n + 1] if base == "past_cap" else [0, 300, 200, n]
    out, osel, obase = _call(ctx, rows, rb)
    assert not obase.any()
    g_rows, g_sel, _ = _guards(n, len(rb) - 1)
    np.testing.assert_array_equal(osel, g_sel)
    for k in SRC:
        np.testing.assert_array_equal(out[k], g_rows[k], err_msg=k)


# ---- argument checks ---------------------------------------------------------------------------------

def test_argument_checks(ctx):
    from _gpu import drp_amd
    n = 100
    rows = {k: _up(v) for k, v in _rows(_uniform(n, 1)).items()}
    out = {k: _up(v) for k, v in _rows(np.zeros(n, np.uint64)).items()}
    base, obase = _up(np.array([0, n], np.uint64)), _up(np.zeros(2, np.uint64))
    sel = _up(np.arange(n, dtype=np.uint64))

    def bad(**kw):
        a = dict(rows=rows, row_base_t=base, nseg=1, rows_cap=n, out_rows=out, out_base_t=obase)
        a.update(kw)
        with pytest.raises(drp_amd.DrpError) as e:
            ctx.order_device(**a)
        assert e.value.rc == drp_amd.DRP_E_INVAL, kw

    bad(nseg=0)
    bad(nseg=drp_amd.FANOUT_MAX + 1)
    bad(rows=None)
    bad(row_base_t=None)
    bad(out_rows=None)
    bad(out_base_t=None)
    bad(out_sel_idx_t=sel)  # (without sel_idx)
    bad(out_rows=dict(out, change=rows["change"]))  # in place
    bad(flags=2)
    bad(flags=0x80000001)
    bad(rows_cap=2**32)
    ctx.order_device(rows, base, 1, n, out, obase)  # (the same arguments as they stand are accepted)
    assert list(_down(obase)) == [0, n]


# ---- determinism -------------------------------------------------------------------------------------

def test_deterministic(ctx):
    n = 3 * TILE + 11
    change = np.random.default_rng(6).integers(0, 300, size=n, dtype=np.uint64)
    rows, base = _rows(change), [0, 1000, 1000, 2 * TILE, n]
    a = _call(ctx, rows, base, limit=[5000, 7, 3000, None], keep_ties=True)
    b = _call(ctx, rows, base, limit=[5000, 7, 3000, None], keep_ties=True)
    for k in SRC:
        np.testing.assert_array_equal(a[0][k], b[0][k], err_msg=k)
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(a[2], b[2])


# ---- end to end through the store ----------------------------------------------------------------------

def _wire(changes):
    return b"".join(S.frame(S.change_payload(k, ch, fr, to, value=v, subset=sub)) for k, sub, ch, fr, to, v in changes)


def _decode(wire):
    """(Changes in wire order, the oracle's columns of the wire)."""
    if not wire:
        return [], None
    ref = O.decode_batch(wire)
    n = ref["nframes"]
    assert ref["err_code"] == 0 and ref["consumed"] == len(wire) and np.all(ref["type"][:n] == 1)
    return [change_at(wire, ref, i) for i in range(n)], ref


def _reorder(wire):
    """The oracle's encoding of the wire's Changes in ascending change, ties in wire order."""
    if not wire:
        return b""
    _, ref = _decode(wire)
    n = ref["nframes"]
    order = np.argsort(ref["change"][:n].astype(np.uint64), kind="stable")
    cols = {k: ref[k][:n][order] for k in ["key_len", "subset_len", "value_len", "change", "from", "to"]}
    for k in ["key", "subset", "value"]:
        cols[k + "_off"] = (ref["payload_off"][:n] + ref[k + "_off"][:n].astype(np.uint64))[order]
    cols["flags"] = (ref["flags"][:n] & 3)[order]
    return O.encode_changes(wire, cols)


@pytest.fixture(scope="module")
def store(ctx):
    """About 3,000 keys from two merged batches: the second brings new keys with small changes and
    rewrites old keys with greater ones, so row order and change order disagree; changes come from a
    range of 60, so many keys tie."""
    import torch
    from _gpu import drp_amd
    rng = np.random.default_rng(31)
    b1 = [(b"key-%04d" % k, b"s" if k % 5 == 0 else None, int(rng.integers(10, 40)), k % 100, k % 7,
           b"v%d" % k if k % 3 else None) for k in range(2000)]
    b2 = [(b"key-%04d" % k, b"s" if k % 5 == 0 else None, int(rng.integers(0, 30)) + (30 if k < 2000 else 0), 1, 2,
           b"w%d" % k) for k in range(1000, 3000)]
    st = drp_amd.Store(ctx, 3500, 1 << 18)
    for batch in [b1, b2]:
        wire = _wire(batch)
        g = ctx.decode_staged(wire)
        n = g["nframes"]
        assert n == len(batch)
        cols = {k: _up(g[k][:n]) for k in ["payload_off", "payload_len", "type", "flags"] + O.COLS32 + O.COLS64}
        st.merge_device(torch.from_numpy(np.frombuffer(wire, np.uint8).copy()).to("cuda:0"), cols, n)
    info = st.query()
    assert info.rows == 3000 and not info.refused
    ch = _down(st.cols["change"])[:3000]
    assert np.any(ch[:-1] > ch[1:])  # row order is not change order
    return st


def _filters(T=(None, 24, None)):
    from _gpu import drp_amd
    specs = [{}, {}, {"key_prefix": b"key-1"}]
    for s, t in zip(specs, T):
        if t is not None:
            s["change_range"] = (t + 1, U64MAX)
    return [drp_amd.make_filter(**s) if s else None for s in specs]


def test_store_catch_up(ctx, store):
    """K = 3 filters (all, change > 24, a key prefix), limit=None: each output holds the same Changes
    as Store.fanout's for that filter, in non-decreasing change, and its bytes are the oracle's
    encoding of fanout's rows in the expected order."""
    plain = store.fanout(_filters())
    got = store.catch_up(_filters(), limit=None)
    assert len(got) == 3
    for f, ((wire, sent, last), ref) in enumerate(zip(got, plain)):
        a, b = _decode(wire)[0], _decode(ref)[0]
        assert sent == len(a) == len(b) > 100, f
        assert collections.Counter(a) == collections.Counter(b), f
        chs = [c.change for c in a]
        assert chs == sorted(chs) and last == chs[-1], f
        assert wire == _reorder(ref), f
    assert len(_decode(got[0][0])[0]) == 3000 and min(c.change for c in _decode(got[1][0])[0]) == 25


def test_store_paging(ctx, store):
    """The paging loop with limit=100, keep_ties=True over three peers at once: send a page, the
    peer's new T is last_change, repeat until every page is empty. It ends, visits every row exactly
    once, and the concatenation of a peer's pages is its limit=None output."""
    whole = [w for w, _, _ in store.catch_up(_filters(), limit=None)]
    T, pages, rounds = [None, 24, None], [[], [], []], 0
    while True:
        rounds += 1
        assert rounds <= 100
        got = store.catch_up(_filters(T), limit=100, keep_ties=True)
        if all(sent == 0 for _, sent, _ in got):
            assert all(w == b"" and last is None for w, _, last in got)
            break
        for f, (w, sent, last) in enumerate(got):
            if sent:
                assert sent >= 100 or b"".join(pages[f]) + w == whole[f]  # (only the last page is short)
                assert T[f] is None or last > T[f]
                pages[f].append(w)
                T[f] = last
    assert rounds > 10
    for f in range(3):
        assert b"".join(pages[f]) == whole[f], f
        a, b = _decode(b"".join(pages[f]))[0], _decode(whole[f])[0]
        assert collections.Counter(a) == collections.Counter(b) and max(collections.Counter(a).values()) == 1
    # exact cuts may end inside a run of ties: the pages are exactly 100 rows
    got = store.catch_up(_filters(), limit=100, keep_ties=False)
    assert [sent for _, sent, _ in got] == [100, 100, 100]
    assert [w for w, _, _ in got] == [_reorder(w)[:len(g[0])] for w, g in zip(store.fanout(_filters()), got)]
