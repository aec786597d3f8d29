"""GPU parity for the merge report (include/drp.h "merge report"): per-row outcomes, the news view
and the stale reply of drp_store_merge_report_device, and the staged forms. The expected side is
test_gpu_store's model of the store (Model, the winners of a batch), extended here to say per batch
row what became of it and which store rows a stale sender lacks; every comparison is bit-exact."""
import random

import numpy as np
import pytest

import _oracle as O
import _streams as S
from _relay import (SRC_KEYS as SRC, U64MAX, change_at as _change, device_cols as _device_cols, make_filter as _filter,
                    mask as _mask)
from test_gpu_store import Model, _blob_stream, _check, _dump, _encode, _pool, _same_raw, _store, _wire

pytestmark = pytest.mark.gpu

NONE, INSERTED, REPLACED, UNCHANGED, STALE, SKIPPED = range(6)
EE = 0xEE


@pytest.fixture(scope="module")
def ctx():
    from _gpu import drp_amd
    c = drp_amd.Ctx(0)
    c.set_blob_skip(drp_amd.BLOB_SKIP_OFF)
    yield c
    c.close()


# ---- the expected side ---------------------------------------------------------------------

def _batch_winners(wire, spec=None, brem=0, bad=()):
    """(n, the oracle's rows, winner rows, winner Changes) of drp_latest_device over the wire's
    delivered rows; `bad`: rows the device columns mark DRP_F_BAD (no candidates)."""
    ref = O.decode_batch(wire, blob_remaining=brem)
    n = ref["nframes"]
    m = _mask(wire, ref, n, spec or {})
    for b in bad:
        m[b] = False
    best = {}
    for i in np.flatnonzero(m):
        c = _change(wire, ref, int(i))
        cur = (c.change, int(i))
        if (c.has, c.subset, c.key) not in best or cur > best[(c.has, c.subset, c.key)][0]:
            best[(c.has, c.subset, c.key)] = (cur, c)
    win = sorted((cur[1], c) for cur, c in best.values())
    return n, ref, [i for i, _ in win], [c for _, c in win]


def _expect(model, wire, spec=None, brem=0, bad=(), skip_rows=()):
    """One merge of `wire` into the model, row by row: {"n", "outcome" (n codes), "news" and
    "news_keep" (the news_type column without and with KEEP_BLOBS), "reply" (the store rows of the
    stale winners, in batch-row order), "reply_changes" (what those rows hold), "cnt" (the record's
    last-merge group), "winners"}."""
    n, ref, rows, changes = _batch_winners(wire, spec, brem, bad)
    outcome, reply = np.zeros(n, np.uint8), []
    for row, c in zip(rows, changes):
        r = model.index.get((c.has, c.subset, c.key))
        if row in skip_rows:
            outcome[row] = SKIPPED
        elif r is None:
            outcome[row] = INSERTED
        elif model.rows[r].change > c.change:
            outcome[row] = STALE
            reply.append(r)
        elif model.rows[r] == c:
            outcome[row] = UNCHANGED
        else:
            outcome[row] = REPLACED
    reply_changes = [model.rows[r] for r in reply]
    cnt = model.merge(changes, skip={j for j, row in enumerate(rows) if row in skip_rows})
    news = np.zeros(n, np.uint8)
    if not cnt["refused"]:
        news[(outcome == INSERTED) | (outcome == REPLACED)] = 1
    keep = news.copy()
    blob = (ref["type"][:n] & 0x3F) == 2
    keep[blob] = ref["type"][:n][blob]
    for k, code in [("inserted", INSERTED), ("replaced", REPLACED), ("unchanged", UNCHANGED), ("stale", STALE),
                    ("skipped", SKIPPED)]:
        assert cnt[k] == int(np.count_nonzero(outcome == code))
    return {"n": n, "outcome": outcome, "news": news, "news_keep": keep, "reply": reply,
            "reply_changes": reply_changes, "cnt": cnt, "winners": rows, "ref": ref}


# ---- the call, with outputs that show every byte written ----------------------------------------

def _filled(nbytes, dtype, off=0):
    """A tensor of `dtype` over nbytes 0xEE bytes, its first element `off` bytes into the allocation."""
    import torch
    return torch.full((nbytes + off + 16,), EE, dtype=torch.uint8, device="cuda:0")[off:off + nbytes].view(dtype)


def _report(ctx, store, wire_t, cols, n, spec=None, keep=False, reply_cap=None, off=(0, 0), pad=64, reply=True):
    """drp_store_merge_report_device with all outputs, every one pre-filled with 0xEE: outcome and
    news_type of n + pad entries (off: their byte offsets into their allocations), the reply's arrays
    of reply_cap (default n) entries. Returns the outputs as numpy arrays."""
    import torch
    from _gpu import drp_amd
    cap = n if reply_cap is None else reply_cap
    outcome, news = _filled(n + pad, torch.uint8, off[0]), _filled(n + pad, torch.uint8, off[1])
    rows = {k: _filled(max(cap, 1) * (4 if k.endswith("_len") else 1 if k == "flags" else 8),
                       torch.int32 if k.endswith("_len") else torch.uint8 if k == "flags" else torch.int64) for k in SRC}
    idx, cnt = _filled(max(cap, 1) * 8, torch.int64), _filled(8, torch.int64)
    ctx.store_merge_report_device(store, wire_t, cols, n, _filter(spec), outcome, news, rows if reply else None,
                                  idx if reply else None, cnt if reply else None, cap if reply else 0,
                                  drp_amd.REPORT_KEEP_BLOBS if keep else 0)
    torch.cuda.synchronize()
    return {"outcome": outcome.cpu().numpy(), "news_type": news.cpu().numpy(),
            "rows": {k: v.cpu().numpy() for k, v in rows.items()}, "rows_t": rows,
            "reply_idx": idx.cpu().numpy().view(np.uint64), "n_reply": int(cnt.cpu()[0]) if reply else None,
            "n_reply_t": cnt}


def _untouched(a, frm=0):
    return bool(np.all(a.view(np.uint8)[frm * a.itemsize:] == EE))


def _check_rows(got, want, n, keep):
    """outcome and news_type of every row, and the entries behind n left as they were."""
    np.testing.assert_array_equal(got["outcome"][:n], want["outcome"])
    np.testing.assert_array_equal(got["news_type"][:n], want["news_keep" if keep else "news"])
    assert _untouched(got["outcome"], n) and _untouched(got["news_type"], n)


def _reply_wire(store, got):
    """The reply's rows encoded with the arena as the heap (Store.reply_bytes over these outputs)."""
    return store.reply_bytes({"reply_rows": got["rows_t"], "n_reply": got["n_reply_t"]})


def _check_reply(store, got, want):
    k = len(want["reply"])
    assert got["n_reply"] == k
    np.testing.assert_array_equal(got["reply_idx"][:k], np.array(want["reply"], np.uint64))
    assert _untouched(got["reply_idx"], k) and all(_untouched(v, k) for v in got["rows"].values())
    assert _reply_wire(store, got) == _encode(want["reply_changes"])


# ---- wires -----------------------------------------------------------------------------------

def _frames(items):
    """items: change tuples as _wire takes them, or bytes (a blob frame)."""
    return b"".join(S.frame(it, 2) if isinstance(it, bytes) else _wire([it]) for it in items)


def _head_and_batch(n, seed, blobs=True):
    """A head batch and a batch of exactly n frames over it: keys from a pool of n // 4, changes from
    a range of 5 (losers inside the batch, inserted, replaced and stale winners), every fifth row a
    winner of the head verbatim (unchanged where it wins its identity) and, with `blobs`, every
    seventh frame a small blob."""
    pool = max(1, n // 4)
    head = _pool(max(1, n // 2), max(1, pool // 2), 5, seed=seed + 7)
    items = _pool(n, pool, 5, seed=seed)
    held = list({(k, sub): (k, sub, ch, fr, to, v) for k, sub, ch, fr, to, v in
                 sorted(head, key=lambda r: r[2])}.values())
    for j in range(0, n, 5):
        items[j] = held[(j // 5) % len(held)]
    if blobs:
        for j in range(3, n, 7):
            items[j] = b"blob%d" % j
    return _wire(head), _frames(items), pool


def _held(ctx, head, max_keys, arena):
    store, model = _store(ctx, max_keys, arena)
    wire_t, cols, n = _device_cols(ctx, head)
    model.merge(_batch_winners(head)[3])
    store.merge_device(wire_t, cols, n, None)
    return store, model


# ---- row counts ------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1025])
def test_row_counts(ctx, n):
    """The wave (64) and the workgroup (256), one below, at and above, 0, 1 and four workgroups and a
    row; merged into a store that holds a head batch. Every row's outcome and news_type, the 64
    entries behind n untouched; KEEP_BLOBS for the odd n."""
    head, wire, pool = _head_and_batch(n, seed=n)
    store, model = _held(ctx, head, 2 * pool + 4, 64 * (n + 4))
    wire_t, cols, rows = _device_cols(ctx, wire)
    assert rows == n
    want = _expect(model, wire)
    got = _report(ctx, store, wire_t, cols, n, keep=bool(n % 2))
    _check_rows(got, want, n, bool(n % 2))
    _check_reply(store, got, want)
    _check(store, model, want["cnt"])
    if n >= 255:
        assert set(want["outcome"].tolist()) == {NONE, INSERTED, REPLACED, UNCHANGED, STALE}
        assert want["reply"] and np.count_nonzero(want["news_keep"] == 2)


def test_odd_offsets(ctx):
    """outcome, news_type and the batch's type column at odd byte offsets (1, 3, 5) into their
    allocations: the 16-byte path's head and tail, with and without KEEP_BLOBS."""
    import torch
    for n, keep in [(1025, True), (257, False), (21, True), (5, True)]:
        head, wire, pool = _head_and_batch(n, seed=300 + n)
        store, model = _held(ctx, head, 2 * pool + 4, 64 * (n + 4))
        wire_t, cols, _ = _device_cols(ctx, wire)
        ty = torch.zeros(n + 32, dtype=torch.uint8, device="cuda:0")[5:5 + n]
        ty.copy_(cols["type"][:n])
        want = _expect(model, wire)
        got = _report(ctx, store, wire_t, {**cols, "type": ty}, n, keep=keep, off=(1, 3))
        _check_rows(got, want, n, keep)
        _check(store, model, want["cnt"])


# ---- every outcome by hand -----------------------------------------------------------------------

def test_every_outcome(ctx):
    """One row of each kind, checked against the model and against the codes written out here."""
    head = [(b"rep-gt", None, 5, 1, 1, b"a"), (b"rep-eq", None, 5, 1, 1, b"a"), (b"same", b"s", 5, 1, 1, b"a"),
            (b"stale", None, 5, 1, 1, b"a"), (b"skip", None, 5, 1, 1, b"a")]
    items = [(b"new", None, 1, 0, 0, b"loser"),       # 0: beaten inside the batch by row 1
             (b"new", None, 2, 0, 0, b"winner"),      # 1: inserted
             (b"rep-gt", None, 6, 1, 1, b"a"),        # 2: replaced by a greater change
             (b"rep-eq", None, 5, 1, 1, b"other"),    # 3: replaced at an equal change, other content
             (b"same", b"s", 5, 1, 1, b"a"),          # 4: unchanged
             (b"stale", None, 4, 1, 1, b"older"),     # 5: stale
             b"a blob",                               # 6: a blob row
             (b"bad", None, 9, 0, 0, b"x"),           # 7: a malformed Change (DRP_F_BAD in the columns)
             (b"skip", None, 7, 1, 1, b"past")]       # 8: skipped (its value range is made to leave the wire)
    wire = _frames(items)
    store, model = _held(ctx, _wire(head), 16, 1 << 12)
    wire_t, cols, n = _device_cols(ctx, wire)
    assert n == len(items)
    cols = {k: v.clone() for k, v in cols.items()}
    cols["flags"][7] |= 4
    cols["value_len"][8] = len(wire) - int(cols["payload_off"][8]) - int(cols["value_off"][8]) + 1
    want = _expect(model, wire, bad=(7,), skip_rows=(8,))
    assert want["outcome"].tolist() == [NONE, INSERTED, REPLACED, REPLACED, UNCHANGED, STALE, NONE, NONE, SKIPPED]
    got = _report(ctx, store, wire_t, cols, n, keep=True)
    _check_rows(got, want, n, True)
    assert got["news_type"][:n].tolist() == [0, 1, 1, 1, 0, 0, 2, 0, 0]
    _check_reply(store, got, want)
    assert want["reply"] == [3] and got["rows"]["change"][0] == 5
    _check(store, model, want["cnt"])
    assert model.rows[4].change == 5  # (the skipped winner's identity keeps what it had)


# ---- reply -----------------------------------------------------------------------------------

def test_reply(ctx):
    """640 winners, the stale ones at winner positions 0, 255, 256, 511, 512 and 639: the scanned
    workgroup counts and the rank inside a workgroup both cross a boundary. The batch holds only
    unchanged and stale winners, so every merge of it classifies alike."""
    from _gpu import drp_amd
    nw, stale = 640, [0, 255, 256, 511, 512, 639]
    head = [(b"key-%04d" % ((i * 37) % nw), b"s" if i % 3 == 0 else None, 10, i % 100, 1, b"value-%d" % i)
            for i in range(nw)]
    order = list(range(nw))
    random.Random(3).shuffle(order)
    batch = [head[i] for i in order]
    for p in stale:
        k, sub, ch, fr, to, v = batch[p]
        batch[p] = (k, sub, 9 - p % 3, fr, to, b"older")
    store, model = _held(ctx, _wire(head), nw, 1 << 16)
    wire = _wire(batch)
    wire_t, cols, n = _device_cols(ctx, wire)
    want = _expect(model, wire)
    assert want["winners"] == list(range(nw)) and np.flatnonzero(want["outcome"] == STALE).tolist() == stale
    assert want["reply"] == [order[p] for p in stale] and not want["news"].any()
    got = _report(ctx, store, wire_t, cols, n)
    _check_rows(got, want, n, False)
    _check_reply(store, got, want)
    # the Store helper: the same rows, and its bytes
    rep = store.merge_report(wire_t, cols, n, reply=True)
    assert int(rep["n_reply"].cpu()[0]) == 6 and rep["reply_idx"].cpu().numpy()[:6].tolist() == want["reply"]
    np.testing.assert_array_equal(rep["outcome"].cpu().numpy(), want["outcome"])
    assert store.reply_bytes(rep) == _encode(want["reply_changes"])
    # one entry short: the true count, nothing written; exactly enough: as before
    got = _report(ctx, store, wire_t, cols, n, reply_cap=5)
    assert got["n_reply"] == 6 and _untouched(got["reply_idx"]) and all(_untouched(v) for v in got["rows"].values())
    got = _report(ctx, store, wire_t, cols, n, reply_cap=6)
    _check_reply(store, got, want)
    # no stale row: 0
    fresh = _wire([(k, sub, 10, fr, to, v) for k, sub, ch, fr, to, v in head[::2]])
    wire_t, cols, n = _device_cols(ctx, fresh)
    want = _expect(model, fresh)
    got = _report(ctx, store, wire_t, cols, n)
    assert got["n_reply"] == 0 and not want["reply"] and _untouched(got["reply_idx"])
    _check_rows(got, want, n, False)
    assert drp_amd.MERGE_STALE == STALE


# ---- refused ---------------------------------------------------------------------------------

def test_refused(ctx):
    """test_capacity's sizing, one row or 16 bytes short: the outcomes as classified, news_type all
    0 or, with KEEP_BLOBS, the blob rows alone, the reply as the model says, the store's raw dump
    as before."""
    first = _wire(_pool(100, 30, 4, seed=1))
    changes = _pool(300, 90, 4, seed=2, first=10)
    items = []
    for j, c in enumerate(changes):
        items.append(c)
        if j % 50 == 20:
            items.append(b"blob-%d" % j)
    wire = _frames(items)
    probe = Model(1 << 20, 1 << 30)
    probe.merge(_batch_winners(first)[3])
    cnt = probe.merge(_batch_winners(wire)[3])
    assert cnt["inserted"] > 20 and cnt["replaced"] > 2 and cnt["stale"] > 2
    idents, bytes_needed = len(probe.rows), probe.used
    for max_keys, arena in [(idents - 1, bytes_needed), (idents, bytes_needed - 16)]:
        store, model = _held(ctx, first, max_keys, arena)
        before = _dump(store)[3]
        wire_t, cols, n = _device_cols(ctx, wire)
        for keep in [False, True]:
            want = _expect(model, wire)
            assert want["cnt"]["refused"] == 1 and not want["news"].any()
            assert np.count_nonzero(want["outcome"] == INSERTED) > 20 and np.count_nonzero(want["news_keep"] == 2) == 6
            got = _report(ctx, store, wire_t, cols, n, keep=keep)
            _check_rows(got, want, n, keep)
            _check_reply(store, got, want)
            info, after = _check(store, model, want["cnt"])
            assert info.refused == 1 and info.merges == 1
            _same_raw(before, after)


# ---- hash masks ------------------------------------------------------------------------------

def test_hash_masks(ctx):
    """The hash cut to 0, 1 and 7 bits: the same report and the same store for each."""
    head, wire, pool = _head_and_batch(300, seed=77)
    res = []
    try:
        for mask in [0, 1, 7]:
            ctx.set_latest_hash_mask(mask)
            store, model = _held(ctx, head, 2 * pool + 4, 1 << 15)
            wire_t, cols, n = _device_cols(ctx, wire)
            want = _expect(model, wire)
            got = _report(ctx, store, wire_t, cols, n, keep=True)
            _check_rows(got, want, n, True)
            _check_reply(store, got, want)
            _, raw = _check(store, model, want["cnt"])
            res.append((got, raw))
    finally:
        ctx.set_latest_hash_mask(U64MAX)
    for got, raw in res[1:]:
        for k in ["outcome", "news_type", "reply_idx"]:
            np.testing.assert_array_equal(got[k], res[0][0][k])
        for k in SRC:
            np.testing.assert_array_equal(got["rows"][k], res[0][0]["rows"][k])
        _same_raw(raw, res[0][1], table=False)


# ---- the relay property --------------------------------------------------------------------------

def test_relay_property(ctx):
    """X and Y start equal. B into X with a report, the news view of B into Y: they hold the same
    rows. B into X again: no news, every winner unchanged (B holds no stale winner)."""
    head = _pool(200, 60, 5, seed=31)
    b = [(k, sub, ch + 4, fr, to, v) for k, sub, ch, fr, to, v in _pool(400, 120, 5, seed=32)]
    held = {(k, sub): (k, sub, ch, fr, to, v) for k, sub, ch, fr, to, v in sorted(head, key=lambda r: r[2])}
    b += [r for r in list(held.values())[::4] if r[2] >= 4][:10]
    items = []
    for j, c in enumerate(b):
        items.append(c)
        if j % 90 == 5:
            items.append(b"blob")
    wire = _frames(items)
    x, model = _held(ctx, _wire(head), 300, 1 << 15)
    y, _ = _held(ctx, _wire(head), 300, 1 << 15)
    wire_t, cols, n = _device_cols(ctx, wire)
    want = _expect(model, wire)
    assert not want["reply"] and want["cnt"]["inserted"] > 20 and want["cnt"]["replaced"] > 20
    rep = x.merge_report(wire_t, cols, n, keep_blobs=True)
    np.testing.assert_array_equal(rep["news_type"].cpu().numpy(), want["news_keep"])
    y.merge_device(wire_t, {**cols, "type": rep["news_type"]}, n)
    _, raw_x = _check(x, model, want["cnt"])
    iy, _, _, raw_y = _dump(y)
    _same_raw(raw_x, raw_y, table=False)
    assert (iy.inserted, iy.replaced, iy.winners) == (want["cnt"]["inserted"], want["cnt"]["replaced"],
                                                      want["cnt"]["inserted"] + want["cnt"]["replaced"])
    again = _expect(model, wire)
    rep = x.merge_report(wire_t, cols, n)
    assert not rep["news_type"].cpu().numpy().any() and not again["news"].any()
    out = rep["outcome"].cpu().numpy()
    np.testing.assert_array_equal(out, again["outcome"])
    assert set(out[again["winners"]].tolist()) == {UNCHANGED}


# ---- the merge itself is unchanged ----------------------------------------------------------------

def test_merge_unchanged(ctx):
    """The same batches through merge_device into one store and through the report call, all outputs
    asked for, into its twin; once more with a NULL report: columns, arena and record identical."""
    wires = [_wire(_pool(300, 80, 6, seed=s, subsets=(None, b"s", b""))) for s in [61, 62, 63, 61]]
    a, model = _store(ctx, 300, 1 << 15)
    b, _ = _store(ctx, 300, 1 << 15)
    c, _ = _store(ctx, 300, 1 << 15)
    for w in wires:
        wire_t, cols, n = _device_cols(ctx, w)
        want = _expect(model, w)
        a.merge_device(wire_t, cols, n, None)
        got = _report(ctx, b, wire_t, cols, n, keep=True)
        ctx.store_merge_report_device(c, wire_t, cols, n, report=False)
        _check_rows(got, want, n, True)
        ia, raw_a = _check(a, model, want["cnt"])
        for other in [b, c]:
            io, _, _, raw_o = _dump(other)
            assert io.as_dict() == ia.as_dict()
            _same_raw(raw_a, raw_o, table=False)
    assert model.seen["replaced_gt"] and model.seen["stale"] and model.seen["unchanged"]


# ---- fan-out over the news view -------------------------------------------------------------------

SPECS = [{"change_range": (3, 6)}, {"subset": b"s"}, {"key_prefix": b"key-1"}]


def _keep(c, spec):
    lo, hi = spec.get("change_range", (0, U64MAX))
    return (lo <= c.change <= hi and ("subset" not in spec or (c.has and c.subset == spec["subset"]))
            and c.key.startswith(spec.get("key_prefix", b"")))


def _news_outputs(want, wire, specs):
    """Per filter, the oracle's encoding of the news rows the filter keeps, in row order, and the
    rows themselves."""
    rows = [int(r) for r in np.flatnonzero(want["news"])]
    kept = [[r for r in rows if _keep(_change(wire, want["ref"], r), spec)] for spec in specs]
    return [_encode([_change(wire, want["ref"], r) for r in rs]) for rs in kept], kept


def test_fanout_over_news(ctx):
    """Three filters (a change range, a subset, a key prefix) over the news view of a batch with blob
    frames between its Changes: output f is the filter over the news rows, the splice table lists the
    batch's blobs with ranks counted over the news rows."""
    import torch
    head, wire, pool = _head_and_batch(700, seed=91)
    store, model = _held(ctx, head, 2 * pool + 4, 1 << 16)
    wire_t, cols, n = _device_cols(ctx, wire)
    want = _expect(model, wire)
    rep = store.merge_report(wire_t, cols, n, keep_blobs=True)
    np.testing.assert_array_equal(rep["news_type"].cpu().numpy(), want["news_keep"])
    outs, kept = _news_outputs(want, wire, SPECS)
    assert all(len(k) > 3 for k in kept) and len(set(map(tuple, kept))) == 3
    K, dev = len(SPECS), wire_t.device
    rows = {k: torch.zeros(K * n, dtype=(torch.int32 if k.endswith("_len") else torch.uint8 if k == "flags" else
                                         torch.int64), device=dev) for k in SRC}
    base, sel = torch.zeros(K + 1, dtype=torch.int64, device=dev), torch.zeros(K * n, dtype=torch.int64, device=dev)
    blobs = [int(r) for r in np.flatnonzero((want["ref"]["type"][:n] & 0x3F) == 2)]
    splice = {"blob_row": torch.zeros(len(blobs), dtype=torch.int64, device=dev),
              "blob_rank": torch.zeros(K * len(blobs), dtype=torch.int64, device=dev),
              "n_blobs": torch.zeros(1, dtype=torch.int64, device=dev)}
    ctx.fanout_device(wire_t, {**cols, "type": rep["news_type"]}, n, [_filter(s) for s in SPECS], rows, K * n, sel,
                      base, splice)
    assert store._encode_outputs(rows, base, wire_t, K) == outs
    rb = base.cpu().numpy()
    for f in range(K):
        assert sel.cpu().numpy()[rb[f]:rb[f + 1]].tolist() == kept[f]
    assert int(splice["n_blobs"].cpu()[0]) == len(blobs) > 50
    assert splice["blob_row"].cpu().numpy().tolist() == blobs
    rank = splice["blob_rank"].cpu().numpy().reshape(K, len(blobs))
    for f in range(K):
        assert rank[f].tolist() == [sum(1 for r in kept[f] if r < b) for b in blobs]
    # the hub step over the same rows (a twin store)
    twin, _ = _held(ctx, head, 2 * pool + 4, 1 << 16)
    info, relayed = twin.relay_news(wire_t, cols, n, [_filter(s) for s in SPECS])
    assert relayed == outs and info.inserted + info.replaced == int(np.count_nonzero(want["news"]))


# ---- staged ----------------------------------------------------------------------------------

def test_staged(ctx):
    """merge_news_staged then fanout_news_staged give Store.relay_news's bytes over the same rows: a
    plain wire, and a wire with blobs staged whole and in blob-skipping pieces. Too small a cap:
    DRP_E_CAPACITY with the size needed, and that size then succeeds with the same bytes. No news
    held (no merge yet, a new stage): DRP_E_INVAL."""
    from _gpu import drp_amd
    big = _blob_stream()
    plain = _wire(_pool(400, 80, 5, seed=4))
    head = _wire(_pool(100, 80, 5, seed=5))
    filters = lambda: [_filter(s) for s in SPECS]
    try:
        for wire, mode in [(plain, drp_amd.BLOB_SKIP_OFF), (big, drp_amd.BLOB_SKIP_OFF),
                           (big, drp_amd.BLOB_SKIP_ALWAYS)]:
            ctx.set_blob_skip(drp_amd.BLOB_SKIP_OFF)
            ref, model = _held(ctx, head, 256, 1 << 14)
            got = _held(ctx, head, 256, 1 << 14)[0]
            wire_t, cols, n = _device_cols(ctx, wire)
            want = _expect(model, wire)
            outs, kept = _news_outputs(want, wire, SPECS)
            info, relayed = ref.relay_news(wire_t, cols, n, filters())
            assert relayed == outs and any(outs) and want["cnt"]["replaced"] and want["cnt"]["inserted"]
            _, raw = _check(ref, model, want["cnt"])
            ctx.set_blob_skip(mode)
            ctx.decode_staged(wire)
            if mode == drp_amd.BLOB_SKIP_ALWAYS:
                assert ctx.timing().h2d_skipped > 0  # (it was staged in pieces)
            with pytest.raises(drp_amd.DrpError) as e:  # (a new stage: the earlier round's news is gone)
                ctx.fanout_news_staged(filters())
            assert e.value.rc == drp_amd.DRP_E_INVAL
            i2 = ctx.store_merge_news_staged(got)
            assert {k: getattr(i2, k) for k in want["cnt"]} == want["cnt"]
            _same_raw(raw, _dump(got)[3], table=False)
            staged, nsel, sp = ctx.fanout_news_staged(filters(), splice=True)
            assert staged == outs and nsel == [len(k) for k in kept]
            blobs = [int(r) for r in np.flatnonzero((want["ref"]["type"][:n] & 0x3F) == 2)]
            assert sp["n_blobs"] == len(blobs) and sp["blob_row"].tolist() == blobs
            for f in range(len(SPECS)):
                ends = np.cumsum([0] + [len(_encode([_change(wire, want["ref"], r)])) for r in kept[f]])
                assert sp["blob_pos"][f].tolist() == [int(ends[sum(1 for r in kept[f] if r < b)]) for b in blobs]
            need = sum(len(o) for o in outs)
            with pytest.raises(drp_amd.DrpError) as e:
                ctx.fanout_news_staged(filters(), cap=need - 1)
            assert e.value.rc == drp_amd.DRP_E_CAPACITY and e.value.written == need
            assert ctx.fanout_news_staged(filters(), cap=need)[0] == outs
            # the plain fan-out of the staged batch is what it was: every Change, news or not
            assert sum(ctx.fanout_staged([None])[1]) == int(np.count_nonzero((want["ref"]["type"][:n] & 0x3F) == 1))
            # a refused merge: every output empty, the blobs still listed
            tiny = drp_amd.Store(ctx, 1, 16)
            with pytest.raises(drp_amd.DrpError) as e:
                ctx.store_merge_news_staged(tiny)
            assert e.value.rc == drp_amd.DRP_E_CAPACITY
            empty, nsel, sp = ctx.fanout_news_staged(filters(), splice=True)
            assert empty == [b""] * 3 and nsel == [0, 0, 0] and sp["n_blobs"] == len(blobs)
    finally:
        ctx.set_blob_skip(drp_amd.BLOB_SKIP_OFF)
    with drp_amd.Ctx(0) as fresh:
        fresh.decode_staged(plain)
        with pytest.raises(drp_amd.DrpError) as e:  # (a staged batch, but no merge has kept its news)
            fresh.fanout_news_staged([None])
        assert e.value.rc == drp_amd.DRP_E_INVAL
        assert sum(fresh.fanout_staged([None])[1]) == 400


# ---- DRP_E_INVAL -----------------------------------------------------------------------------

def test_invalid(ctx):
    """Unknown flag bits, news_type aliasing the batch's type column, reply_rows without n_reply, a
    NULL array in reply_rows with reply_cap > 0; the store is not touched."""
    import torch
    from _gpu import drp_amd
    wire = _wire(_pool(50, 10, 3, seed=8))
    store, model = _held(ctx, wire, 32, 1 << 12)
    before = _dump(store)[3]
    wire_t, cols, n = _device_cols(ctx, wire)
    z = lambda dt: torch.zeros(n, dtype=dt, device=wire_t.device)
    rows = {k: z(torch.int32 if k.endswith("_len") else torch.uint8 if k == "flags" else torch.int64) for k in SRC}
    cnt = torch.zeros(1, dtype=torch.int64, device=wire_t.device)
    bad = [dict(outcome_t=z(torch.uint8), flags=2), dict(outcome_t=z(torch.uint8), flags=0x80000001),
           dict(news_type_t=cols["type"]), dict(reply_rows=rows, reply_cap=n),
           dict(reply_rows={**rows, "to": None}, n_reply_t=cnt, reply_cap=n)]
    for kw in bad:
        with pytest.raises(drp_amd.DrpError) as e:
            ctx.store_merge_report_device(store, wire_t, cols, n, **kw)
        assert e.value.rc == drp_amd.DRP_E_INVAL, kw.keys()
    # (a NULL array is fine while reply_cap is 0: only the count is written)
    ctx.store_merge_report_device(store, wire_t, cols, n, reply_rows={**rows, "to": None}, n_reply_t=cnt, reply_cap=0)
    assert int(cnt.cpu()[0]) == 0
    _same_raw(before, _dump(store)[3])
