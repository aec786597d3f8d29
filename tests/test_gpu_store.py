"""GPU parity for the store (drp_store_*): the latest Change per (subset presence, subset bytes, key
bytes) over every batch merged so far, resident on the device in the layout of a decoded batch.
Every comparison is bit-exact against an expected side built here on the CPU: the oracle's decode of
each wire, the select predicate in numpy, the per-batch winners (greatest change, then greatest
row), and a model of the store: a dict from identity to row, the rows in the order their identities
entered, the arena offsets and the counters of include/drp.h "store"."""
import collections
import random

import numpy as np
import pytest

import _oracle as O
import _streams as S
from _relay import (U64MAX, Change, bytes_at as _bytes_at, device_cols as _device_cols, make_filter as _filter,
                    wire_winners as _winners)

pytestmark = pytest.mark.gpu

COUNTERS = ["winners", "inserted", "replaced", "unchanged", "stale", "skipped"]


@pytest.fixture(scope="module")
def ctx():
    from _gpu import drp_amd
    c = drp_amd.Ctx(0)
    c.set_blob_skip(drp_amd.BLOB_SKIP_OFF)
    yield c
    c.close()


# ---- the expected side (the predicate, the winners and the Change tuple: _relay) -------------

def _r16(n):
    return (n + 15) & ~15


def _plen(c):
    return len(c.key) + len(c.subset) + len(c.value)


class Model:
    """The store's contract: merge(winners) applies one merge, all or nothing."""

    def __init__(self, max_keys, arena_bytes):
        self.max_keys, self.arena_bytes = max_keys, arena_bytes
        self.rows, self.offs, self.index = [], [], {}
        self.used = self.dead = self.merges = 0
        self.seen = collections.Counter()  # outcomes over the store's life, replaced split by cause

    def merge(self, winners, skip=()):
        cnt = dict.fromkeys(COUNTERS, 0)
        cnt["winners"] = len(winners)
        plan, need, dead, kinds = [], 0, 0, []
        for j, c in enumerate(winners):
            if j in skip:
                cnt["skipped"] += 1
                continue
            r = self.index.get((c.has, c.subset, c.key))
            if r is None:
                cnt["inserted"] += 1
                kinds.append("inserted")
            elif self.rows[r].change > c.change:
                cnt["stale"] += 1
                kinds.append("stale")
                continue
            elif self.rows[r] == c:
                cnt["unchanged"] += 1
                kinds.append("unchanged")
                continue
            else:
                cnt["replaced"] += 1
                kinds.append("replaced_gt" if c.change > self.rows[r].change else "replaced_eq")
                dead += _r16(_plen(self.rows[r]))
            plan.append((r, c, self.used + need))
            need += _r16(_plen(c))
        cnt["need_rows"], cnt["need_bytes"] = cnt["inserted"], need
        cnt["refused"] = int(len(self.rows) + cnt["inserted"] > self.max_keys or self.used + need > self.arena_bytes)
        if cnt["refused"]:
            return cnt
        self.seen.update(kinds)
        for r, c, off in plan:
            if r is None:
                self.index[(c.has, c.subset, c.key)] = len(self.rows)
                self.rows.append(c)
                self.offs.append(off)
            else:
                self.rows[r], self.offs[r] = c, off
        self.used += need
        self.dead += dead
        self.merges += 1
        return cnt

    def compact(self):
        at = 0
        for r, c in enumerate(self.rows):
            self.offs[r] = at
            at += _r16(_plen(c))
        self.used, self.dead = at, 0


def _dump(store):
    """The record, the rows in use as (Changes, offsets) with the stored form checked, and the raw
    columns, arena and table."""
    info = store.query()
    cols = {k: v.cpu().numpy() for k, v in store.cols.items()}
    arena = store.arena.cpu().numpy()[:store.arena_bytes]
    n = info.rows
    assert n <= store.max_keys and info.arena_used <= store.arena_bytes
    assert np.all(cols["type"][:n] == 1) and np.all(cols["type"][n:store.max_keys] == 0)
    rows, offs = [], []
    for r in range(n):
        kl, sl, vl = int(cols["key_len"][r]), int(cols["subset_len"][r]), int(cols["value_len"][r])
        po, fl = int(cols["payload_off"][r]), int(cols["flags"][r])
        assert po % 16 == 0 and po + _r16(kl + sl + vl) <= info.arena_used, r
        assert int(cols["payload_len"][r]) == kl + sl + vl and fl & ~3 == 0, r
        assert (int(cols["key_off"][r]), int(cols["subset_off"][r]), int(cols["value_off"][r])) == (0, kl, kl + sl), r
        assert (fl & 1 or sl == 0) and (fl & 2 or vl == 0), r
        assert not arena[po + kl + sl + vl:po + _r16(kl + sl + vl)].any(), r  # the allocation's tail
        b = _bytes_at(arena, po, kl + sl + vl)
        rows.append(Change(bool(fl & 1), b[kl:kl + sl], b[:kl], int(np.uint64(cols["change"][r])),
                           int(np.uint64(cols["from"][r])), int(np.uint64(cols["to"][r])), bool(fl & 2), b[kl + sl:]))
        offs.append(po)
    return info, rows, offs, (cols, arena, store.table.cpu().numpy())


def _check(store, model, cnt=None):
    info, rows, offs, raw = _dump(store)
    assert rows == model.rows
    assert offs == model.offs
    assert (info.rows, info.arena_used, info.arena_dead, info.merges) == (len(model.rows), model.used, model.dead,
                                                                         model.merges)
    if cnt is not None:
        got = info.as_dict()
        assert {k: got[k] for k in cnt} == cnt
    return info, raw


def _same_raw(a, b, table=True):
    """Two dumps hold the same columns and arena and, for two states of one store, the same table
    (two stores may differ there: which of two colliding identities claimed the earlier slot)."""
    for x, y in zip(a[0].values(), b[0].values()):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(a[1], b[1])
    if table:
        np.testing.assert_array_equal(a[2], b[2])
    else:
        assert np.count_nonzero(a[2]) == np.count_nonzero(b[2])


# ---- wires and their device columns ---------------------------------------------------------

def _wire(changes):
    """changes: (key, subset or None, change, from, to, value or None)."""
    return b"".join(S.frame(S.change_payload(k, ch, fr, to, value=v, subset=sub)) for k, sub, ch, fr, to, v in changes)


def _pool(n, pool, changes, seed, subsets=(None, None, b"s"), first=0):
    """n rows over keys key-<first .. first + pool); from / to / value tell the rows of a key apart."""
    rng = random.Random(seed)
    return [(b"key-%d" % (first + rng.randrange(pool)), rng.choice(subsets), rng.randrange(changes), r % 128,
             (r * 7) % 128, b"%d" % r if r % 3 else None) for r in range(n)]


def _store(ctx, max_keys, arena_bytes):
    from _gpu import drp_amd
    return drp_amd.Store(ctx, max_keys, arena_bytes), Model(max_keys, arena_bytes)


def _merge(ctx, store, model, wire, spec=None, skip=()):
    """One merge_device of `wire` into store and model; the store is compared with the model."""
    wire_t, cols, n = _device_cols(ctx, wire)
    cnt = model.merge(_winners(wire, spec)[1], skip)
    store.merge_device(wire_t, cols, n, _filter(spec))
    return _check(store, model, cnt), cnt


# ---- row counts ------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025])
def test_row_counts(ctx, n):
    """0, 1, and the wave (64), merge workgroup (256: four of them at 1024) and select workgroup
    (1024) sizes, one below, at and above; keys from a pool of n // 4 and changes from a range of 5.
    Into an empty store, and again into one that holds half the pool."""
    pool = max(1, n // 4)
    wire = _wire(_pool(n, pool, 5, seed=n))
    store, model = _store(ctx, 2 * pool + 4, 64 * (n + 4))
    (_, _), cnt = _merge(ctx, store, model, wire)
    assert cnt["inserted"] == cnt["winners"] and (n < 63 or 0 < cnt["winners"] < n)
    store, model = _store(ctx, 2 * pool + 4, 64 * (n + 4))
    half = _wire(_pool(max(1, n // 2), max(1, pool // 2), 5, seed=n + 7))
    _merge(ctx, store, model, half)
    (_, _), cnt = _merge(ctx, store, model, wire)
    if n >= 63:
        assert cnt["inserted"] and cnt["replaced"] + cnt["unchanged"] + cnt["stale"]


# ---- outcomes --------------------------------------------------------------------------------

def test_outcomes(ctx):
    """Every outcome at least twice, the counters against the model's, the store against the winners
    of the concatenation (property 9), and once against drp_latest_device over the concatenated
    wire."""
    import torch
    rng = random.Random(5)
    base = _pool(200, 60, 6, seed=50)
    b2 = []
    for j, (k, sub, ch, fr, to, v) in enumerate(_winner_rows(base)):
        kind = j % 5
        if kind == 0:
            b2.append((k, sub, ch, fr, to, v))            # unchanged
        elif kind == 1:
            b2.append((k, sub, ch + 9, fr, to, v))        # replaced by a greater change
        elif kind == 2:
            b2.append((k, sub, ch, fr, to, b"other%d" % j))  # replaced on an equal change
        elif kind == 3 and ch > 0:
            b2.append((k, sub, ch - 1, fr, to, v))        # stale
    b2 += _pool(120, 30, 6, seed=51, first=1000)          # inserted
    rng.shuffle(b2)
    b3 = _pool(200, 90, 12, seed=52, first=20) + b2[:40]
    b4 = [(k, sub, ch, to, fr, v) for k, sub, ch, fr, to, v in b3[::3]] + _pool(150, 50, 20, seed=53, first=980)
    wires = [_wire(b) for b in [base, b2, b3, b4]]
    store, model = _store(ctx, 700, 1 << 16)
    for w in wires:
        _merge(ctx, store, model, w)
    for kind in ["inserted", "replaced_gt", "replaced_eq", "unchanged", "stale"]:
        assert model.seen[kind] >= 2, (kind, model.seen)
    assert model.dead > 0
    # property 9, against the expected side: the concatenation's winners, by identity
    whole = b"".join(wires)
    want = {(c.has, c.subset, c.key): c for c in _winners(whole)[1]}
    info, rows, _, _ = _dump(store)
    assert {(c.has, c.subset, c.key): c for c in rows} == want and len(rows) == len(want)
    # and against drp_latest_device over the concatenated wire
    wire_t, cols, n = _device_cols(ctx, whole)
    dev = wire_t.device
    out = {k: torch.zeros(n, dtype=(torch.int32 if k.endswith("_len") else torch.uint8 if k == "flags" else
                                    torch.int64), device=dev)
           for k in ["key_off", "key_len", "subset_off", "subset_len", "value_off", "value_len", "change", "from", "to",
                     "flags"]}
    nsel_t = torch.zeros(1, dtype=torch.int64, device=dev)
    ctx.latest_device(wire_t, cols, n, None, out, None, nsel_t)
    torch.cuda.synchronize()
    nsel = int(nsel_t.cpu()[0])
    o = {k: v.cpu().numpy()[:nsel] for k, v in out.items()}
    got = {}
    for i in range(nsel):
        fl = int(o["flags"][i])
        f = lambda k: _bytes_at(whole, o[k + "_off"][i], o[k + "_len"][i])
        c = Change(bool(fl & 1), f("subset") if fl & 1 else b"", f("key"), int(np.uint64(o["change"][i])),
                   int(np.uint64(o["from"][i])), int(np.uint64(o["to"][i])), bool(fl & 2), f("value") if fl & 2 else b"")
        got[(c.has, c.subset, c.key)] = c
    assert got == want


def _winner_rows(rows):
    """The rows of `rows` (tuples as _wire takes them) that win their identity."""
    best = {}
    for r, (k, sub, ch, fr, to, v) in enumerate(rows):
        if (k, sub) not in best or (ch, r) > best[(k, sub)][0]:
            best[(k, sub)] = ((ch, r), rows[r])
    return [row for _, row in sorted(best.values())]


# ---- identity edges --------------------------------------------------------------------------

def test_identity_edges(ctx):
    """An absent against a present empty subset, "a" against "ab", the empty key; keys and values of
    7, 8, 9, 15, 16 and 17 bytes (the tails of the eight-byte compares and the sixteen-byte copies),
    a 4 KB value (sixteen steps of the copy) and one of 4097 bytes, a Change with no value. Merged
    twice with other values (every identity is found again: replaced), then once more (unchanged)."""
    lens = [7, 8, 9, 15, 16, 17]
    rows = [(b"same", None, 3, 1, 2, b"x"), (b"same", b"", 3, 1, 2, b"x"), (b"same", b"s", 3, 1, 2, None),
            (b"a", None, 1, 0, 0, b""), (b"ab", None, 1, 0, 0, None), (b"", None, 1, 0, 0, b"empty key"),
            (b"", b"", 1, 0, 0, None), (b"a", b"b", 1, 0, 0, b"v"), (b"", b"ab", 1, 0, 0, b"v"),
            (b"big", None, 5, 6, 7, bytes(range(256)) * 16), (b"big+1", None, 5, 6, 7, bytes(range(256)) * 16 + b"!")]
    for n in lens:
        key = bytes(range(65, 65 + n))
        rows += [(key, None, 2, 0, 0, b"val")]
        rows += [(key[:-1] + b"!", key, 2, 0, 0, bytes(range(97, 97 + n)))]
        rows += [(b"v%d" % n, None, 2, 0, 0, bytes(range(48, 48 + n)))]
    assert len({(k, sub) for k, sub, *_ in rows}) == len(rows)
    store, model = _store(ctx, len(rows), 1 << 15)
    (_, _), cnt = _merge(ctx, store, model, _wire(rows))
    assert cnt["inserted"] == len(rows)
    # the same identities, the value's last byte changed (or a value given / taken away)
    other = [(k, sub, ch, fr, to, (v[:-1] + b"~") if v else (b"now" if v is None else None))
             for k, sub, ch, fr, to, v in rows]
    (_, _), cnt = _merge(ctx, store, model, _wire(other[::-1]))
    assert cnt["replaced"] == len(rows) and cnt["inserted"] == 0
    (_, _), cnt = _merge(ctx, store, model, _wire(other))
    assert cnt["unchanged"] == len(rows)


def test_idempotence(ctx):
    """The same batch twice: the second merge finds every winner unchanged and takes no arena."""
    wire = _wire(_pool(500, 120, 5, seed=9, subsets=(None, b"s", b"")))
    store, model = _store(ctx, 400, 1 << 15)
    (info, raw), cnt = _merge(ctx, store, model, wire)
    (info2, raw2), cnt2 = _merge(ctx, store, model, wire)
    assert cnt2["unchanged"] == cnt2["winners"] == cnt["inserted"] > 100
    assert info2.arena_used == info.arena_used and info2.merges == 2
    _same_raw(raw, raw2)


# ---- hash masks ------------------------------------------------------------------------------

def test_hash_masks(ctx):
    """The hash cut to 0, 1 and 3 bits, and whole: with mask 0 every identity starts at one slot, one
    probe chain through all of them and a byte compare at every step of a lookup. Columns, arena and
    record are identical for every mask (the table is not: it is where the mask shows)."""
    rng = random.Random(40)
    idents = [(b"key%02d" % (k // 2), None if k % 2 else b"x") for k in range(60)]
    mk = lambda seed, n: [(*rng.choice(idents), rng.randrange(6), r % 100, seed, b"%d" % r if r % 4 else None)
                          for r in range(n)]
    wires = [_wire(mk(1, 170)), _wire(mk(2, 170)), _wire(mk(3, 170))]
    raws = []
    try:
        for mask in [0, 1, 7, U64MAX]:
            ctx.set_latest_hash_mask(mask)
            store, model = _store(ctx, 64, 1 << 14)
            for w in wires:
                (info, raw), _ = _merge(ctx, store, model, w)
            assert info.rows > 40 and model.seen["replaced_gt"] and model.seen["stale"]
            raws.append(raw)
    finally:
        ctx.set_latest_hash_mask(U64MAX)
    for raw in raws[1:]:
        for k in raws[0][0]:
            np.testing.assert_array_equal(raw[0][k], raws[0][0][k], err_msg=k)
        np.testing.assert_array_equal(raw[1], raws[0][1])


# ---- filters ---------------------------------------------------------------------------------

@pytest.mark.parametrize("spec", [{"change_range": (2, 4)}, {"subset": b"tt"}, {"key_prefix": b"key-1"}])
def test_filters(ctx, spec):
    """Only the rows the filter keeps enter: the winners are the filtered rows' (a key whose latest
    change lies beyond the range enters with its last change inside it)."""
    rows = _pool(600, 70, 7, seed=6, subsets=(None, b"s", b"tt", b""))
    store, model = _store(ctx, 300, 1 << 14)
    (info, _), cnt = _merge(ctx, store, model, _wire(rows), spec)
    assert 4 < cnt["inserted"] < len(_winners(_wire(rows))[1])
    (info, _), cnt = _merge(ctx, store, model, _wire(_pool(600, 70, 7, seed=7, subsets=(None, b"s", b"tt", b""))), spec)
    assert cnt["inserted"] + cnt["replaced"] + cnt["stale"] + cnt["unchanged"] == cnt["winners"] > 4


# ---- capacity --------------------------------------------------------------------------------

def test_capacity(ctx):
    """max_keys and the arena exactly as large as the batch needs: it fits. One row or 16 bytes
    fewer: refused, with the columns, arena, table and record's totals byte-identical to before, the
    needs as the model has them and DRP_E_CAPACITY from merge_staged; a smaller batch then fits."""
    from _gpu import drp_amd
    first = _wire(_pool(100, 30, 4, seed=1))
    wire = _wire(_pool(300, 90, 4, seed=2, first=10))
    small = _wire(_pool(20, 5, 4, seed=3, first=10))
    probe = Model(1 << 20, 1 << 30)
    probe.merge(_winners(first)[1])
    idents, bytes_needed = len(probe.rows), probe.used
    cnt = probe.merge(_winners(wire)[1])
    assert cnt["inserted"] > 20 and cnt["replaced"] > 2
    idents, bytes_needed = len(probe.rows), probe.used
    for max_keys, arena, fits in [(idents, bytes_needed, True), (idents - 1, bytes_needed, False),
                                  (idents, bytes_needed - 16, False)]:
        store, model = _store(ctx, max_keys, arena)
        (_, before), _ = _merge(ctx, store, model, first)
        (info, after), cnt = _merge(ctx, store, model, wire)
        assert info.refused == cnt["refused"] == (0 if fits else 1)
        assert (info.need_rows, info.need_bytes) == (cnt["need_rows"], cnt["need_bytes"])
        if fits:
            assert info.rows == max_keys and info.arena_used == arena
            continue
        _same_raw(before, after)
        assert info.merges == 1
        ctx.decode_staged(wire)
        with pytest.raises(drp_amd.DrpError) as e:
            store.merge_staged()
        assert e.value.rc == drp_amd.DRP_E_CAPACITY
        assert e.value.info.refused == 1 and e.value.info.need_bytes == cnt["need_bytes"]
        _same_raw(before, _dump(store)[3])
        (info, _), cnt = _merge(ctx, store, model, small)
        assert info.refused == 0 and info.merges == 2 and cnt["winners"] > 0


# ---- wire bounds -----------------------------------------------------------------------------

def test_wire_bounds(ctx):
    """One winner's value_len, in the device columns, made to reach past the wire's end: the merge
    never reads that value, counts the winner as skipped and merges the rest. Once for a new
    identity, once for one the store holds (it keeps what it had)."""
    rows = [(b"key%03d" % i, None, i % 5 + 1, 1, 2, b"value%d" % i) for i in range(130)]
    wire = _wire(rows)
    store, model = _store(ctx, 200, 1 << 14)
    for bad in [70, 3]:
        wire_t, cols, n = _device_cols(ctx, wire)
        cols = {k: v.clone() for k, v in cols.items()}
        cols["value_len"][bad] = len(wire) - int(cols["payload_off"][bad]) - int(cols["value_off"][bad]) + 1
        winners = _winners(wire)[1]
        if bad == 3:  # a second delivery with greater changes: all replaced but the skipped one
            winners = [c._replace(change=c.change + 10) for c in winners]
            cols["change"] += 10
        cnt = model.merge(winners, skip={bad})
        store.merge_device(wire_t, cols, n, None)
        _check(store, model, cnt)
        assert cnt["skipped"] == 1 and cnt["inserted"] + cnt["replaced"] == 129
    assert model.rows[3].change == rows[3][2] and model.rows[2].change == rows[2][2] + 10


# ---- staged ----------------------------------------------------------------------------------

def _blob_stream():
    """Units of 150 Changes over a small key pool and one 300 KB blob, long enough for the stage step
    to cut the batch into pieces that skip blob payload; the keys repeat across the pieces."""
    rng = random.Random(11)
    parts = []
    for u in range(5):
        parts.append(_wire([(k, sub, ch + u, fr, to, v) for k, sub, ch, fr, to, v in _pool(150, 60, 4, seed=20 + u)]))
        parts.append(S.frame(rng.randbytes(300000), 2))
    return b"".join(parts)


def test_staged(ctx):
    """merge_staged gives the store merge_device gives over the same rows: a plain wire, a wire with
    blobs staged whole and in blob-skipping pieces, and one that starts inside a blob. No staged
    batch: DRP_E_INVAL."""
    from _gpu import drp_amd
    big = _blob_stream()
    plain = _wire(_pool(400, 80, 5, seed=4))
    with drp_amd.Ctx(0) as fresh:
        st = drp_amd.Store(fresh, 8, 256)
        with pytest.raises(drp_amd.DrpError) as e:
            st.merge_staged()
        assert e.value.rc == drp_amd.DRP_E_INVAL
    try:
        for wire, brem, mode in [(plain, 0, drp_amd.BLOB_SKIP_OFF), (big, 0, drp_amd.BLOB_SKIP_OFF),
                                 (big, 0, drp_amd.BLOB_SKIP_ALWAYS),
                                 (random.Random(1).randbytes(1001) + big, 1001, drp_amd.BLOB_SKIP_ALWAYS)]:
            ctx.set_blob_skip(drp_amd.BLOB_SKIP_OFF)
            ref, model = _store(ctx, 256, 1 << 14)
            # both stores first hold `head`, so the staged merge meets more than insertions
            head = _wire(_pool(100, 80, 5, seed=5))
            _merge(ctx, ref, model, head)
            wire_t, cols, n = _device_cols(ctx, wire, brem)
            cnt = model.merge(_winners(wire, None, brem)[1])
            ref.merge_device(wire_t, cols, n, None)
            _, want = _check(ref, model, cnt)
            got, model2 = _store(ctx, 256, 1 << 14)
            _merge(ctx, got, model2, head)
            ctx.set_blob_skip(mode)
            ctx.decode_staged(wire, blob_remaining=brem)
            if mode == drp_amd.BLOB_SKIP_ALWAYS:
                assert ctx.timing().h2d_skipped > 0  # (it was staged in pieces)
            info = got.merge_staged()
            assert {k: getattr(info, k) for k in cnt} == cnt and cnt["replaced"] and cnt["inserted"]
            _same_raw(want, _dump(got)[3], table=False)
    finally:
        ctx.set_blob_skip(drp_amd.BLOB_SKIP_OFF)


# ---- compact ---------------------------------------------------------------------------------

def test_compact(ctx):
    """After merges that left dead bytes: a compact into an arena that is too small is refused and
    the store intact; one that fits leaves arena_dead 0, arena_used the live total, the rows as they
    were but for payload_off, and still found: the last batch again is all unchanged."""
    pools = [_pool(300, 80, 9, seed=s, subsets=(None, b"s")) for s in [1, 2, 3]]
    # (the last batch's changes lie above the others': every one of its winners enters the store)
    pools[2] = [(k, sub, ch + 20, fr, to, v) for k, sub, ch, fr, to, v in pools[2]]
    wires = [_wire(p) for p in pools]
    store, model = _store(ctx, 200, 1 << 15)
    for w in wires:
        (info, before), _ = _merge(ctx, store, model, w)
    assert info.arena_dead > 0
    live = info.arena_used - info.arena_dead
    assert live == sum(_r16(_plen(c)) for c in model.rows)
    i = store.compact(live - 16)
    assert i.refused == 1 and i.need_bytes == live and (i.arena_used, i.arena_dead) == (info.arena_used, info.arena_dead)
    _same_raw(before, _dump(store)[3])
    i = store.compact(live)
    model.compact()
    model.arena_bytes = live
    assert i.refused == 0 and (i.arena_used, i.arena_dead, i.merges) == (live, 0, 3) and store.arena_bytes == live
    _, after = _check(store, model)
    for k in before[0]:
        if k != "payload_off":
            np.testing.assert_array_equal(before[0][k], after[0][k], err_msg=k)
    np.testing.assert_array_equal(before[2], after[2])  # the table maps identities to rows
    # (the new arena is full: a merge that changes nothing still fits)
    (_, _), cnt = _merge(ctx, store, model, wires[-1])
    assert cnt["unchanged"] == cnt["winners"] > 50 and cnt["refused"] == 0


# ---- catch-up --------------------------------------------------------------------------------

def _encode(rows):
    """The oracle's encoding of Changes, in order."""
    heap, cols = bytearray(), {k: [] for k in ["key_off", "key_len", "subset_off", "subset_len", "value_off",
                                                "value_len", "change", "from", "to", "flags"]}
    for c in rows:
        for name, b in [("key", c.key), ("subset", c.subset), ("value", c.value)]:
            cols[name + "_off"].append(len(heap))
            cols[name + "_len"].append(len(b))
            heap += b
        cols["change"].append(c.change)
        cols["from"].append(c.frm)
        cols["to"].append(c.to)
        cols["flags"].append((1 if c.has else 0) | (2 if c.hv else 0))
    arr = {k: np.array(v, np.uint32 if k.endswith("_len") else np.uint8 if k == "flags" else np.uint64)
           for k, v in cols.items()}
    return O.encode_changes(bytes(heap) or b"\0", arr) if rows else b""


@pytest.mark.parametrize("K", [1, 3, 64])
def test_catch_up(ctx, K):
    """Store.fanout, the existing fan-out and encoder over the store's view: K peers at versions
    T_f, some with a subset or a key prefix; output f is the oracle's encoding of the rows with
    change > T_f (and the subset, the prefix) in store order, with n = max_keys and with n = rows."""
    wires = [_wire(_pool(300, 100, 12, seed=s, subsets=(None, b"s", b"tt"))) for s in [11, 12, 13]]
    store, model = _store(ctx, 400, 1 << 15)
    for w in wires:
        _merge(ctx, store, model, w)
    specs = []
    for f in range(K):
        spec = {"change_range": (f % 12 + 1, U64MAX)}
        if f % 4 == 1:
            spec["subset"] = b"s"
        if f % 4 == 2:
            spec["key_prefix"] = b"key-%d" % (f % 9 + 1)
        specs.append(spec)

    def keep(c, spec):
        return (c.change >= spec["change_range"][0] and ("subset" not in spec or (c.has and c.subset == spec["subset"]))
                and c.key.startswith(spec.get("key_prefix", b"")))

    want = [_encode([c for c in model.rows if keep(c, spec)]) for spec in specs]
    assert sum(1 for w in want if w) >= min(K, 3)
    assert store.fanout([_filter(s) for s in specs]) == want
    assert 0 < len(model.rows) < store.max_keys
    assert store.fanout([_filter(s) for s in specs], n=len(model.rows)) == want
