"""GPU parity for the store lifecycle (include/drp.h "store lifecycle"): drp_store_load_device and
drp_store_rehash_device, and Store.grow / retain / state / from_state over them. The expected side is
test_gpu_store's model of the store: a load of rows with distinct new identities is the model's merge
of those rows (all inserted), and a pruned store is the model rebuilt from the kept rows in their old
order. Columns, arena and record are compared bit for bit; tables never are (which of two colliding
identities holds the earlier slot is a race): they are compared through drp_store_lookup_device over
every stored identity and absent ones.

Every store here holds the identity edges: the empty key, keys that differ only in subset presence
(absent against present and empty), values absent, empty and 15, 16, 17 and 4097 bytes long."""
import copy

import numpy as np
import pytest

from _relay import U64MAX, device_cols as _device_cols, make_filter as _filter, wire_winners as _winners
from test_gpu_store import Model, _check, _dump, _merge, _same_raw, _store, _wire

pytestmark = pytest.mark.gpu

ABSENT, LEVEL = 1, 3
LAST = ["winners", "inserted", "replaced", "unchanged", "stale", "skipped", "refused", "need_rows", "need_bytes"]


@pytest.fixture(scope="module")
def ctx():
    from _gpu import drp_amd
    c = drp_amd.Ctx(0)
    c.set_blob_skip(drp_amd.BLOB_SKIP_OFF)
    yield c
    c.set_latest_hash_mask(U64MAX)
    c.close()


# ---- stores to start from ---------------------------------------------------------------------

def _idents(n, first=0):
    """n rows (as _wire takes them) of pairwise distinct identities, the edges first."""
    rows = [(b"", None, 1, 0, 0, b"empty key"), (b"", b"", 1, 0, 0, None), (b"same", None, 3, 1, 2, b"x"),
            (b"same", b"", 3, 1, 2, b""), (b"v15", None, 2, 0, 0, bytes(range(15))), (b"v16", b"s", 2, 0, 0, bytes(range(16))),
            (b"v17", None, 2, 0, 0, bytes(range(17))), (b"big", b"tt", 5, 6, 7, bytes(range(256)) * 16 + b"!")]
    if first:
        rows = []
    subs = (None, b"s", b"tt", b"")
    rows += [(b"key-%04d" % (first + i), subs[i % 4], i % 9 + 1, i % 128, (i * 7) % 128, b"%d" % i if i % 3 else None)
             for i in range(n - len(rows))]
    assert len({(k, sub) for k, sub, *_ in rows}) == len(rows) == n
    return rows


def _build(ctx, n, max_keys=None, arena_bytes=1 << 17):
    """A store of exactly n rows in use, in the order of _idents(n), after three merges (the second
    and third replace, so payloads lie out of row order and arena_dead > 0) and one compact."""
    rows = _idents(n)
    store, model = _store(ctx, n + 7 if max_keys is None else max_keys, arena_bytes)
    _merge(ctx, store, model, _wire(rows[:2 * n // 3]))
    _merge(ctx, store, model, _wire([(k, sub, ch + 10, to, fr, (v or b"") + b"+") for k, sub, ch, fr, to, v in rows[n // 3:]]))
    assert model.dead > 0
    assert store.compact(arena_bytes).refused == 0
    model.compact()
    _merge(ctx, store, model, _wire([(k, sub, ch + 20, fr, to, b"third") for k, sub, ch, fr, to, v in rows[::5]]))
    assert len(model.rows) == n and model.dead > 0
    return store, model


def _rebuilt(rows, max_keys, arena_bytes):
    """The model of a fresh store that one load (or merge) of `rows` (Changes) filled, and its counts."""
    m = Model(max_keys, arena_bytes)
    cnt = m.merge(rows)
    assert cnt["inserted"] == len(rows) or cnt["refused"]
    return m, cnt


def _load(ctx, store, wire_t, cols, n, spec=None, clash=True):
    """store_load_device; returns the clash count (None without the check)."""
    import torch
    clash_t = torch.full((1,), 0x5555, dtype=torch.int64, device="cuda:0") if clash else None
    ctx.store_load_device(store, wire_t, cols, n, _filter(spec), clash_t)
    torch.cuda.synchronize()
    return int(clash_t.cpu()[0]) if clash else None


def _lookups(ctx, store, model, gone=()):
    """The table through the lookup: every identity the model holds is found in its row at its change
    (those of the rows `gone` are absent), and absent identities, some of them a held key under the
    other subset presence, are absent."""
    import torch
    held = [(c.key, c.subset if c.has else None, c.change, 0, 0, None) for c in model.rows]
    absent = [(b"absent-%d" % i, (None, b"", b"s")[i % 3], 1, 0, 0, None) for i in range(6)]
    absent += [(b"v15", b"", 1, 0, 0, None), (b"v16", None, 1, 0, 0, None), (b"", b"s", 1, 0, 0, None)]
    absent = [q for q in absent if (q[1] is not None, q[1] or b"", q[0]) not in model.index]
    wire_t, cols, n = _device_cols(ctx, _wire(held + absent))
    r = store.lookup(wire_t, cols, n, emit=None)
    torch.cuda.synchronize()
    want_v = [ABSENT if j in gone else LEVEL for j in range(len(held))] + [ABSENT] * len(absent)
    want_h = [-1 if j in gone else j for j in range(len(held))] + [-1] * len(absent)
    np.testing.assert_array_equal(r["verdict"].cpu().numpy(), np.array(want_v, np.uint8))
    np.testing.assert_array_equal(r["hit_row"].cpu().numpy(), np.array(want_h, np.int64))


# ---- 1. load equals merge ------------------------------------------------------------------------

@pytest.mark.parametrize("mask", [U64MAX, 0, 1, 7])
@pytest.mark.parametrize("n", [255, 256, 257, 513])
def test_load_equals_merge(ctx, n, mask):
    """The view of a store of n rows (one below, at and above a workgroup of 256, and three of them)
    loaded into A and merged into an identical B: the same columns, arena and record, byte for byte,
    type zero beyond the rows, the same lookups, clash 0; under the whole hash and under 0, 1 and 3
    bits of it (one probe chain through every slot, two, eight), the mask set before any init."""
    from _gpu import drp_amd
    ctx.set_latest_hash_mask(mask)
    try:
        src, model = _build(ctx, n)
        A = drp_amd.Store(ctx, n + 3, 1 << 17)
        B = drp_amd.Store(ctx, n + 3, 1 << 17)
        clash = _load(ctx, A, src._view(), src.cols, src.max_keys)
        B.merge_device(src._view(), src.cols, src.max_keys)
        ia, _, _, raw_a = _dump(A)  # (asserts type == 0 beyond the rows)
        ib, _, _, raw_b = _dump(B)
        _same_raw(raw_a, raw_b, table=False)
        assert bytes(ia) == bytes(ib) and ia.rows == n and ia.inserted == ia.winners == n
        assert clash == 0
        want, cnt = _rebuilt(model.rows, n + 3, 1 << 17)
        _check(A, want, cnt)
        _lookups(ctx, A, want)
        _lookups(ctx, B, want)
    finally:
        ctx.set_latest_hash_mask(U64MAX)


# ---- 2. a filter and a type column: the pruned store ---------------------------------------------

def _named_lack(ctx, src, model, named):
    """lack_type of a lookup that names `named` of the store's identities at their stored change: the
    store's view under it holds every row but those. Returns (the column, the named rows)."""
    n = len(model.rows)
    idx = sorted({(j * 7 + 3) % n for j in range(named)})
    assert len(idx) == named
    q = [(model.rows[j].key, model.rows[j].subset if model.rows[j].has else None, model.rows[j].change, 0, 0, None)
         for j in idx]
    wire_t, cols, nq = _device_cols(ctx, _wire(q))
    return src.lookup(wire_t, cols, nq, emit=None, lack=True)["lack_type"], set(idx)


@pytest.mark.parametrize("spec,named", [({"change_range": (12, 19)}, 0), ({"subset": b"s"}, 0), (None, 1), (None, 64),
                                        (None, 65), ({"change_range": (0, 25)}, 65)])
def test_load_filter_and_type_column(ctx, spec, named):
    """A change range, a subset equality, and the lack_type of a lookup naming 1, 64 and 65 keys (a
    wave of named rows, and one more) in the type column's place: the loaded store is the model
    rebuilt from the kept rows in old row order, rows dense and arena compact. Store.retain gives the
    same store."""
    from _gpu import drp_amd
    n = 300
    src, model = _build(ctx, n)
    view, out = dict(src.cols), set()
    if named:
        view["type"], out = _named_lack(ctx, src, model, named)

    def keep(j, c):
        if j in out:
            return False
        if spec and "change_range" in spec and not spec["change_range"][0] <= c.change <= spec["change_range"][1]:
            return False
        return not (spec and "subset" in spec) or (c.has and c.subset == spec["subset"])

    kept = [c for j, c in enumerate(model.rows) if keep(j, c)]
    assert 10 < len(kept) < n
    want, cnt = _rebuilt(kept, n, 1 << 17)
    A = drp_amd.Store(ctx, n, 1 << 17)
    assert _load(ctx, A, src._view(), view, src.max_keys, spec) == 0
    _check(A, want, cnt)
    _lookups(ctx, A, want)
    # Store.retain: the same store in place of the old one
    i = src.retain(_filter(spec), view["type"] if named else None, max_keys=n, arena_bytes=1 << 17)
    assert i.clash == 0 and i.refused == 0 and i.arena_dead == 0
    _check(src, want, cnt)
    _lookups(ctx, src, want)
    _same_raw(_dump(A)[3], _dump(src)[3], table=False)


# ---- 3. append -----------------------------------------------------------------------------------

def test_append(ctx):
    """A load of a decoded batch (offsets into a wire, not a store's view) into a store that holds
    rows, the identities disjoint: the rows go behind the store's and the payloads behind arena_used,
    as the model's merge puts them; a later merge that replaces old and loaded keys matches the model."""
    store, model = _build(ctx, 200, max_keys=600)
    base_rows, base_used = len(model.rows), model.used
    more = _idents(300, first=5000)
    wire = _wire(more)
    wire_t, cols, n = _device_cols(ctx, wire)
    cnt = model.merge(_winners(wire)[1])
    assert cnt["inserted"] == 300 and cnt["refused"] == 0
    assert _load(ctx, store, wire_t, cols, n) == 0
    info, _ = _check(store, model, cnt)
    assert model.offs[base_rows] == base_used and info.rows == base_rows + 300 and info.merges == 4
    _lookups(ctx, store, model)
    both = _idents(200)[3::4] + more[1::3]
    (_, _), cnt = _merge(ctx, store, model, _wire([(k, sub, ch + 50, fr, to, b"later") for k, sub, ch, fr, to, v in both]))
    assert cnt["replaced"] == len(both) and cnt["inserted"] == 0
    _lookups(ctx, store, model)


# ---- 4. all or nothing ---------------------------------------------------------------------------

def test_all_or_nothing(ctx):
    """max_keys equal to the rows after the load and arena_bytes equal to the need: it fits. One row
    or 16 bytes less: refused = 1, need_rows and need_bytes set, and columns, arena, table and the
    record's totals as before; clash is 0."""
    first = _wire(_idents(100))
    more = _idents(300, first=7000)
    wire = _wire(more)
    probe = Model(1 << 20, 1 << 30)
    probe.merge(_winners(first)[1])
    probe.merge(_winners(wire)[1])
    rows, need = len(probe.rows), probe.used
    for max_keys, arena, fits in [(rows, need, True), (rows - 1, need, False), (rows, need - 16, False)]:
        store, model = _store(ctx, max_keys, arena)
        (_, before), _ = _merge(ctx, store, model, first)
        wire_t, cols, n = _device_cols(ctx, wire)
        cnt = model.merge(_winners(wire)[1])
        clash = _load(ctx, store, wire_t, cols, n)
        info, after = _check(store, model, cnt)
        assert info.refused == cnt["refused"] == (0 if fits else 1) and clash == 0
        assert (info.need_rows, info.need_bytes, info.winners) == (300, cnt["need_bytes"], 300)
        if fits:
            assert info.rows == max_keys and info.arena_used == arena and info.merges == 2
            _lookups(ctx, store, model)
        else:
            _same_raw(before, after)
            assert info.merges == 1


# ---- 5. clash --------------------------------------------------------------------------------------

def _dup(row, j):
    k, sub, ch, fr, to, v = row
    return (k, sub, ch + j, fr, to, b"dup%d" % j)


@pytest.mark.parametrize("mask", [U64MAX, 0])
@pytest.mark.parametrize("case", ["two_and_three", "held", "both"])
def test_clash(ctx, case, mask):
    """Two rows of one identity and three of another inside the load (in different workgroups), an
    identity the store holds, and both: clash = loaded rows - new distinct identities, the same over
    three runs (which of the duplicates holds the earlier slot is a race; the count is not), and with
    every identity in one probe chain (hash mask 0)."""
    held = _idents(20)
    rows = _idents(300, first=9000)
    if case in ("two_and_three", "both"):
        rows = rows[:290] + [_dup(rows[2], 1)] + rows[290:] + [_dup(rows[7], 1), _dup(rows[7], 2)]
    if case in ("held", "both"):
        rows = rows[:100] + [_dup(held[1], 1)] + rows[100:]  # ("" under a present, empty subset)
    new = {(k, sub) for k, sub, *_ in rows} - {(k, sub) for k, sub, *_ in held}
    want = len(rows) - len(new)
    assert want == {"two_and_three": 3, "held": 1, "both": 4}[case]
    wire = _wire(rows)
    ctx.set_latest_hash_mask(mask)
    try:
        for _ in range(3):
            store, model = _store(ctx, 400, 1 << 16)
            _merge(ctx, store, model, _wire(held))
            wire_t, cols, n = _device_cols(ctx, wire)
            assert _load(ctx, store, wire_t, cols, n) == want
            info = store.query()
            assert (info.refused, info.winners, info.inserted, info.rows) == (0, len(rows), len(rows), 20 + len(rows))
    finally:
        ctx.set_latest_hash_mask(U64MAX)


# ---- 6. skipped ------------------------------------------------------------------------------------

def test_skipped(ctx):
    """One selected row whose value range ends one byte past nbytes (the wire is the head of a larger
    tensor, so a wrong read stays inside the allocation): the row counts as skipped and is never
    stored, the other rows load."""
    import torch
    rows = _idents(130)
    wire = _wire(rows)
    wire_t, cols, n = _device_cols(ctx, wire)
    padded = torch.cat([wire_t, torch.full((64,), 0xEE, dtype=torch.uint8, device=wire_t.device)])
    bad = 70
    cols = {k: v.clone() for k, v in cols.items()}
    cols["value_len"][bad] = len(wire) - int(cols["payload_off"][bad]) - int(cols["value_off"][bad]) + 1
    assert int(cols["flags"][bad]) & 2
    store, model = _store(ctx, 200, 1 << 15)
    cnt = model.merge(_winners(wire)[1], skip={bad})
    assert _load(ctx, store, padded[:len(wire)], cols, n) == 0
    _check(store, model, cnt)
    assert cnt["skipped"] == 1 and cnt["inserted"] == 129
    _lookups(ctx, store, model)


# ---- 7. rehash -------------------------------------------------------------------------------------

def _rehash(ctx, store, report=True):
    import torch
    rep = torch.full((2,), 0x5555, dtype=torch.int64, device="cuda:0") if report else None
    ctx.store_rehash_device(store, rep)
    torch.cuda.synchronize()
    return [int(v) for v in rep.cpu()] if report else None


def _totals(info):
    return (info.rows, info.arena_used, info.arena_dead, info.merges)


def test_rehash_rebuilds_the_table(ctx):
    """After merges and a compact: a rehash leaves columns, arena and the record's totals alone,
    zeroes the last-merge group, reports [0, 0], and the lookups are as before; over a table of random
    words (with and without a report) it is right again, and a further merge matches the model."""
    import torch
    store, model = _build(ctx, 300)
    before_info, _, _, before = _dump(store)
    _lookups(ctx, store, model)
    assert _rehash(ctx, store) == [0, 0]
    info, _, _, after = _dump(store)
    _same_raw(before, after, table=False)
    assert _totals(info) == _totals(before_info) and all(getattr(info, k) == 0 for k in LAST)
    _lookups(ctx, store, model)
    for report in [True, False]:
        store.table.random_(-2**62, 2**62)
        assert _rehash(ctx, store, report) == ([0, 0] if report else None)
        assert torch.count_nonzero(store.table).item() == 300
        _lookups(ctx, store, model)
    _merge(ctx, store, model, _wire(_idents(300)[1::2] + _idents(5, first=4000)))
    _lookups(ctx, store, model)


def test_rehash_under_another_mask(ctx):
    """A store filled under hash mask 0, the ctx's mask then set to all ones: after a rehash the store
    lives under the new mask: lookups, and a further merge against the model."""
    ctx.set_latest_hash_mask(0)
    try:
        store, model = _build(ctx, 257)
        ctx.set_latest_hash_mask(U64MAX)
        assert _rehash(ctx, store) == [0, 0]
        _lookups(ctx, store, model)
        (_, _), cnt = _merge(ctx, store, model, _wire([(k, sub, ch + 40, fr, to, b"masked") for k, sub, ch, fr, to, v in
                                                       _idents(257)[::3]] + _idents(4, first=4000)))
        assert cnt["replaced"] == 86 and cnt["inserted"] == 4
        _lookups(ctx, store, model)
    finally:
        ctx.set_latest_hash_mask(U64MAX)


def test_rehash_reports_a_corrupt_row(ctx):
    """Row 3's payload_off set to arena_bytes (the declared size; the tensor is larger): report[0] is
    1, refused is 1, and the row is unreachable by lookup while every other row is found."""
    store, model = _build(ctx, 40, arena_bytes=1 << 14)
    store.arena_bytes = int(store.query().arena_used)
    assert store.arena.numel() > store.arena_bytes and int(store.cols["payload_len"][3]) > 0
    store.cols["payload_off"][3] = store.arena_bytes
    assert _rehash(ctx, store) == [1, 0]
    assert store.query().refused == 1
    _lookups(ctx, store, model, gone={3})


def test_rehash_reports_duplicate_rows(ctx):
    """Two rows of one identity (row 7 made a copy of row 5): report[1] is 1 and refused is 1."""
    store, model = _build(ctx, 40, arena_bytes=1 << 14)
    for v in store.cols.values():
        v[7] = v[5]
    assert _rehash(ctx, store) == [0, 1]
    assert store.query().refused == 1


# ---- 8. Python: grow, state / from_state, retain -------------------------------------------------

def test_grow_max_keys(ctx):
    """300 keys, all in use: a merge with new keys is refused; after grow(max_keys=1000) it is
    accepted and matches the model; the rows kept their index and the arena was not touched."""
    store, model = _build(ctx, 300, max_keys=300)
    more = _wire(_idents(150, first=3000) + [(k, sub, ch + 60, fr, to, b"grown") for k, sub, ch, fr, to, v in _idents(300)[::7]])
    (info, before), cnt = _merge(ctx, store, model, more)
    assert info.refused == cnt["refused"] == 1
    arena = store.arena
    with pytest.raises(ValueError):
        store.grow(max_keys=299)
    i = store.grow(max_keys=1000)
    model.max_keys = 1000
    assert store.max_keys == 1000 and store.arena is arena and i.refused == 0 and _totals(i) == _totals(info)
    _, after = _check(store, model)
    for k in before[0]:
        np.testing.assert_array_equal(before[0][k], after[0][k][:300], err_msg=k)
    _lookups(ctx, store, model)
    (info, _), cnt = _merge(ctx, store, model, more)
    assert info.refused == 0 and cnt["inserted"] == 150 and cnt["replaced"] == 43
    _lookups(ctx, store, model)


def test_grow_arena(ctx):
    """An arena with no room for the next merge: refused; after grow(arena_bytes=...) accepted, the
    table and the columns untouched."""
    store, model = _build(ctx, 120, max_keys=400)
    used = int(store.query().arena_used)
    assert store.compact(used - model.dead).refused == 0  # (an arena exactly as large as the live bytes)
    model.compact()
    model.arena_bytes = store.arena_bytes
    more = _wire(_idents(50, first=3000))
    (info, _), cnt = _merge(ctx, store, model, more)
    assert info.refused == cnt["refused"] == 1
    table = store.table
    with pytest.raises(ValueError):
        store.grow(arena_bytes=store.arena_bytes - 16)
    store.grow(arena_bytes=1 << 16)
    model.arena_bytes = 1 << 16
    assert store.table is table and store.arena_bytes == 1 << 16
    _check(store, model)
    (info, _), cnt = _merge(ctx, store, model, more)
    assert info.refused == 0 and cnt["inserted"] == 50
    _lookups(ctx, store, model)


def test_state_round_trip(ctx):
    """state() -> from_state() on a second store: the same dump, the same first-level digest at 4
    bits, and a following merge behaves identically on both."""
    import torch
    from _gpu import drp_amd
    store, model = _build(ctx, 257, max_keys=400, arena_bytes=1 << 16)
    st = store.state()
    assert sorted(st) == ["arena", "arena_dead", "arena_used", "cols", "merges", "rows"]
    assert all(isinstance(v, np.ndarray) and len(v) == 257 for v in st["cols"].values())
    assert len(st["arena"]) == model.used and (st["rows"], st["arena_dead"], st["merges"]) == (257, model.dead, model.merges)
    twin = drp_amd.Store.from_state(ctx, st, max_keys=400, arena_bytes=1 << 16)
    ia, rows_a, offs_a, raw_a = _dump(store)
    ib, rows_b, offs_b, raw_b = _dump(twin)
    assert rows_a == rows_b == model.rows and offs_a == offs_b and _totals(ia) == _totals(ib)
    _same_raw(raw_a, raw_b, table=False)
    assert torch.equal(store.digest(4), twin.digest(4))
    _lookups(ctx, twin, model)
    wire = _wire([(k, sub, ch + 30, fr, to, b"after") for k, sub, ch, fr, to, v in _idents(257)[::2]] + _idents(9, first=2000))
    twin_model = copy.deepcopy(model)
    (_, ra), ca = _merge(ctx, store, model, wire)
    (_, rb), cb = _merge(ctx, twin, twin_model, wire)
    assert ca == cb and ca["replaced"] == 129 and ca["inserted"] == 9
    _same_raw(ra, rb, table=False)
    # the default sizes are what the state uses; a state that does not fit is refused on the host
    small = drp_amd.Store.from_state(ctx, st)
    assert (small.max_keys, small.arena_bytes) == (257, len(st["arena"]))
    _lookups(ctx, small, _holding(rows_a))
    with pytest.raises(ValueError):
        drp_amd.Store.from_state(ctx, st, max_keys=256)
    dup = dict(st, cols={k: v.copy() for k, v in st["cols"].items()})
    for v in dup["cols"].values():
        v[7] = v[5]
    with pytest.raises(drp_amd.DrpError):
        drp_amd.Store.from_state(ctx, dup)


def _holding(rows):
    """A model that holds `rows` (Changes) in order, for _lookups (which reads rows and index only)."""
    m = Model(len(rows), 0)
    m.rows = list(rows)
    m.index = {(c.has, c.subset, c.key): r for r, c in enumerate(rows)}
    return m


def test_retain_refused_or_clashing_leaves_the_store(ctx):
    """retain into a store one row too small is refused, and retain of a store that holds two rows of
    one identity clashes: either way the record says so and the store keeps its tensors, byte for
    byte."""
    store, model = _build(ctx, 100)
    tensors = (store.arena, store.table, store.info, store.cols)
    before = _dump(store)[3]
    i = store.retain(max_keys=99)
    assert i.refused == 1 and i.need_rows == 100 and i.clash == 0
    assert all(a is b for a, b in zip((store.arena, store.table, store.info, store.cols), tensors))
    assert store.max_keys == 107
    _same_raw(before, _dump(store)[3])
    _check(store, model)
    for v in store.cols.values():
        v[7] = v[5]
    before = _dump(store)[3]
    i = store.retain()
    assert i.refused == 0 and i.clash == 1
    assert store.arena is tensors[0] and store.table is tensors[1] and store.info is tensors[2]
    _same_raw(before, _dump(store)[3])
