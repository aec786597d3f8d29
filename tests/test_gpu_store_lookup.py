"""GPU parity for the lookup (include/drp.h "lookup"): drp_store_lookup_device's verdicts, hit rows,
counts, emitted rows and lack_type column, the staged form and the Store helpers over them (lookup,
get, sync_reply). The expected side is test_gpu_store's model of the store: a query's verdict is
model.index.get(identity) and a compare of `change`, the expected bytes are the oracle's encoding of
the model's rows; every comparison is bit-exact. The queries are read here from host copies of the
very columns the device gets, so hand-made columns (a DRP_F_BAD mark, a range that leaves the wire)
are modelled by the same code as decoded ones."""
import random

import numpy as np
import pytest

import _streams as S
from _relay import SRC_KEYS as SRC, U64MAX, device_cols as _device_cols, make_filter as _filter, mask as _mask
from test_gpu_store import Model, _blob_stream, _dump, _encode, _merge, _pool, _same_raw, _store, _wire

pytestmark = pytest.mark.gpu

NONE, ABSENT, BEHIND, LEVEL, AHEAD = range(5)
FOUND = (BEHIND, LEVEL, AHEAD)
AA, PAD, M64 = 0xAA, 64, 2**64


@pytest.fixture(scope="module")
def ctx():
    from _gpu import drp_amd
    c = drp_amd.Ctx(0)
    c.set_blob_skip(drp_amd.BLOB_SKIP_OFF)
    yield c
    c.close()


# ---- the expected side ---------------------------------------------------------------------

def _host(cols):
    """The device columns as unsigned numpy arrays."""
    un = {np.dtype(np.int64): np.uint64, np.dtype(np.int32): np.uint32, np.dtype(np.uint8): np.uint8}
    return {k: (lambda a: a.view(un[a.dtype]))(v.cpu().numpy()) for k, v in cols.items()}


def _query(wire, nbytes, q, i):
    """Row i as a query, ((has, subset, key), change), or None where its key range or (with a
    subset) its subset range leaves [0, nbytes): the device's arithmetic, modulo 2^64."""
    has = bool(int(q["flags"][i]) & 1)
    po = int(q["payload_off"][i])
    koff, klen = (po + int(q["key_off"][i])) % M64, int(q["key_len"][i])
    soff, slen = (po + int(q["subset_off"][i])) % M64, int(q["subset_len"][i]) if has else 0
    inside = lambda off, ln: ln <= nbytes and off <= nbytes - ln
    if not inside(koff, klen) or (has and not inside(soff, slen)):
        return None
    return (has, bytes(wire[soff:soff + slen]) if has else b"", bytes(wire[koff:koff + klen])), int(q["change"][i])


def _expect(model, wire, cols, n, spec=None, emit=FOUND, nbytes=None):
    """What a lookup of rows [0, n) of (wire, cols) in `model` gives: verdict and hit_row per row, the
    five counts, the emitted queries' batch rows ("out_query"), store rows' Changes ("out_changes")
    and columns ("out_cols"), and the lack_type column of max_keys entries."""
    q = _host(cols)
    nbytes = len(wire) if nbytes is None else nbytes
    verdict, hit = np.zeros(n, np.uint8), np.full(n, U64MAX, np.uint64)
    lack = np.zeros(model.max_keys, np.uint8)
    lack[:len(model.rows)] = 1
    for i in np.flatnonzero(_mask(wire, q, n, spec or {})):
        qq = _query(wire, nbytes, q, int(i))
        if qq is None:
            continue
        r = model.index.get(qq[0])
        if r is None:
            verdict[i] = ABSENT
            continue
        held = model.rows[r].change
        verdict[i] = AHEAD if held > qq[1] else LEVEL if held == qq[1] else BEHIND
        hit[i] = r
        if qq[1] >= held:
            lack[r] = 0
    out_query = [i for i in range(n) if verdict[i] in emit]
    out_cols = {k: [] for k in SRC}
    for i in out_query:
        c, off = model.rows[int(hit[i])], model.offs[int(hit[i])]
        for k, v in [("key_off", off), ("key_len", len(c.key)), ("subset_off", off + len(c.key)),
                     ("subset_len", len(c.subset)), ("value_off", off + len(c.key) + len(c.subset)),
                     ("value_len", len(c.value)), ("change", c.change), ("from", c.frm), ("to", c.to),
                     ("flags", (1 if c.has else 0) | (2 if c.hv else 0))]:
            out_cols[k].append(v)
    return {"n": n, "verdict": verdict, "hit": hit, "counts": np.bincount(verdict, minlength=5).astype(np.uint64),
            "out_query": out_query, "out_changes": [model.rows[int(hit[i])] for i in out_query], "out_cols": out_cols,
            "lack": lack}


# ---- the call, with outputs that show every byte written ----------------------------------------

def _dtype(k):
    import torch
    return torch.int32 if k.endswith("_len") else torch.uint8 if k == "flags" else torch.int64


def _filled(count, dtype):
    """A tensor of `count` entries (at least one) whose every byte is 0xAA."""
    import torch
    size = torch.empty(0, dtype=dtype).element_size()
    return torch.full((max(count, 1) * size,), AA, dtype=torch.uint8, device="cuda:0").view(dtype)


def _mask_of(emit):
    m = 0
    for code in emit:
        m |= 1 << code
    return m


def _lookup(ctx, store, wire_t, cols, n, spec=None, emit=FOUND, rows_cap=None, lack=True):
    """drp_store_lookup_device with every output, each pre-filled with 0xAA: verdict and hit_row of
    n + PAD entries, lack_type of max_keys + PAD, the emitted rows' arrays of rows_cap (default n)
    + PAD. Returns the outputs as numpy arrays (and the row tensors)."""
    import torch
    cap = n if rows_cap is None else rows_cap
    verdict, hit, counts = _filled(n + PAD, torch.uint8), _filled(n + PAD, torch.int64), _filled(5, torch.int64)
    lack_t = _filled(store.max_keys + PAD, torch.uint8) if lack else None
    rows = {k: _filled(cap + PAD, _dtype(k)) for k in SRC}
    oq, n_out = _filled(cap + PAD, torch.int64), _filled(1, torch.int64)
    ctx.store_lookup_device(store, wire_t, cols, n, _filter(spec), _mask_of(emit), verdict, hit, counts, lack_t, rows, oq,
                            n_out, cap)
    torch.cuda.synchronize()
    return {"verdict": verdict.cpu().numpy(), "hit": hit.cpu().numpy().view(np.uint64),
            "counts": counts.cpu().numpy().view(np.uint64), "lack": lack_t.cpu().numpy() if lack else None,
            "lack_t": lack_t, "rows": {k: v.cpu().numpy() for k, v in rows.items()}, "rows_t": rows,
            "out_query": oq.cpu().numpy().view(np.uint64), "n_out": int(n_out.cpu()[0]), "n_out_t": n_out, "cap": cap}


def _untouched(a, frm=0):
    return bool(np.all(a.view(np.uint8)[frm * a.itemsize:] == AA))


def _rows_wire(store, got):
    """The emitted rows encoded with the arena as the heap."""
    import torch
    base = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda:0"), got["n_out_t"][:1]])
    return store._encode_outputs(got["rows_t"], base, store._view(), 1)[0]


def _check(store, got, want):
    """Every output against the expected side, and every entry behind the written ones untouched."""
    n, k = want["n"], len(want["out_query"])
    np.testing.assert_array_equal(got["verdict"][:n], want["verdict"])
    np.testing.assert_array_equal(got["hit"][:n], want["hit"])
    assert _untouched(got["verdict"], n) and _untouched(got["hit"], n)
    np.testing.assert_array_equal(got["counts"], want["counts"])
    assert got["n_out"] == k
    if k <= got["cap"]:
        np.testing.assert_array_equal(got["out_query"][:k], np.array(want["out_query"], np.uint64))
        for c in SRC:
            un = got["rows"][c].view({8: np.uint64, 4: np.uint32, 1: np.uint8}[got["rows"][c].itemsize])
            np.testing.assert_array_equal(un[:k], np.array(want["out_cols"][c], un.dtype), err_msg=c)
        assert _untouched(got["out_query"], k) and all(_untouched(v, k) for v in got["rows"].values())
        assert _rows_wire(store, got) == _encode(want["out_changes"])
    else:
        assert _untouched(got["out_query"]) and all(_untouched(v) for v in got["rows"].values())
    if got["lack"] is not None:
        np.testing.assert_array_equal(got["lack"][:store.max_keys], want["lack"])
        assert _untouched(got["lack"], store.max_keys)


# ---- the store most tests share (a lookup writes nothing into it) ---------------------------------

HELD = [(b"key-%d" % i, (None, None, b"s", b"tt")[i % 4], 5 + i % 7, i % 128, (i * 7) % 128, b"%d" % i if i % 3 else None)
        for i in range(300)]


@pytest.fixture(scope="module")
def held(ctx):
    """300 identities in a store of 320 rows: key-i, every fourth under subset "s", every fourth under
    "tt", changes 5 .. 11."""
    store, model = _store(ctx, 320, 1 << 15)
    _merge(ctx, store, model, _wire(HELD))
    assert len(model.rows) == 300
    return store, model


def _have(n, seed, held_rows=HELD):
    """n queries (Changes without a value): about half name a held identity, with a change one
    below, at or one above the stored one; the others a key the store does not hold."""
    rng = random.Random(seed)
    rows = []
    for _ in range(n):
        if rng.random() < 0.5:
            k, sub, ch, _, _, _ = rng.choice(held_rows)
            rows.append((k, sub, ch + rng.choice([-1, 0, 1]), 0, 0, None))
        else:
            rows.append((b"nokey-%d" % rng.randrange(1000), rng.choice([None, b"s"]), rng.randrange(12), 0, 0, None))
    return rows


# ---- row counts ------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 513, 1025])
def test_row_counts(ctx, held, n):
    """0, 1, the wave (64) and the workgroup (256), one below, at and above, and two and four
    workgroups and a row (the scan of the workgroups' emitted counts). Present and absent keys in a
    seeded pattern, the change below, at and above the stored one; all three bits emitted."""
    store, model = held
    wire = _wire(_have(n, seed=n))
    wire_t, cols, rows = _device_cols(ctx, wire)
    assert rows == n
    want = _expect(model, wire, cols, n)
    _check(store, _lookup(ctx, store, wire_t, cols, n), want)
    if n >= 63:
        assert all(want["counts"][c] for c in [ABSENT, BEHIND, LEVEL, AHEAD])


# ---- each emit_mask ----------------------------------------------------------------------------

@pytest.mark.parametrize("emit", [(BEHIND,), (LEVEL,), (AHEAD,), (BEHIND, LEVEL), (BEHIND, AHEAD), (LEVEL, AHEAD)])
def test_emit_masks(ctx, held, emit):
    store, model = held
    wire = _wire(_have(300, seed=77))
    wire_t, cols, n = _device_cols(ctx, wire)
    want = _expect(model, wire, cols, n, emit=emit)
    assert 0 < len(want["out_query"]) < n
    _check(store, _lookup(ctx, store, wire_t, cols, n, emit=emit), want)


# ---- verdict edges -----------------------------------------------------------------------------

def test_verdict_edges(ctx):
    """Stored changes 0, 1, 2^32 - 1, 2^32, 2^63 and 2^64 - 1, queried one below, at and one above
    where such a number exists: the compare is unsigned and 64 bits wide."""
    edges = [0, 1, 2**32 - 1, 2**32, 2**63, U64MAX]
    store, model = _store(ctx, 8, 1 << 10)
    _merge(ctx, store, model, _wire([(b"edge%d" % j, None, c, 1, 2, b"v") for j, c in enumerate(edges)]))
    rows, expect = [], []
    for j, c in enumerate(edges):
        for qc, code in [(c - 1, AHEAD), (c, LEVEL), (c + 1, BEHIND)]:
            if 0 <= qc <= U64MAX:
                rows.append((b"edge%d" % j, None, qc, 0, 0, None))
                expect.append(code)
    assert len(rows) == 16
    wire = _wire(rows)
    wire_t, cols, n = _device_cols(ctx, wire)
    want = _expect(model, wire, cols, n)
    assert want["verdict"].tolist() == expect
    _check(store, _lookup(ctx, store, wire_t, cols, n), want)


# ---- identity edges ----------------------------------------------------------------------------

def test_identity_edges(ctx):
    """The empty key, "a" against "ab"; keys of 7, 8, 9, 15, 16, 17 and 33 bytes against keys that
    differ only in the last and only in the first byte (the ends of the eight-byte compares); one key
    without a subset, with an empty one and under "s"; one key under two subsets."""
    lens = [7, 8, 9, 15, 16, 17, 33]
    longs = [bytes(range(65, 65 + L)) for L in lens]
    stored = [(b"", None), (b"a", None), (b"ab", None), (b"same", None), (b"same", b""), (b"same", b"s"),
              (b"two", b"x"), (b"two", b"y")] + [(k, None) for k in longs] + [(longs[2], longs[3])]
    store, model = _store(ctx, 32, 1 << 12)
    _merge(ctx, store, model, _wire([(k, sub, 3, 1, 2, b"val%d" % j) for j, (k, sub) in enumerate(stored)]))
    absent = [(b"b", None), (b"abc", None), (b"", b""), (b"a", b""), (b"ab", b"a"), (b"same", b"t"), (b"same", b"ss"),
              (b"two", None), (b"two", b"z"), (b"sam", b"e"), (longs[3], longs[2])]
    for k in longs:
        absent += [(k[:-1] + b"!", None), (b"!" + k[1:], None), (k + b"!", None)]
    assert not set(absent) & set(stored)
    rows = [(k, sub, 3, 0, 0, None) for k, sub in stored + absent]
    random.Random(3).shuffle(rows)
    wire = _wire(rows)
    wire_t, cols, n = _device_cols(ctx, wire)
    want = _expect(model, wire, cols, n)
    assert want["counts"].tolist() == [0, len(absent), 0, len(stored), 0]
    _check(store, _lookup(ctx, store, wire_t, cols, n), want)


# ---- duplicates and lack_type --------------------------------------------------------------------

@pytest.mark.parametrize("pair,lacks", [((-1, +1), False), ((+1, -1), False), ((-1, -1), True)])
def test_duplicates_and_lack_type(ctx, held, pair, lacks):
    """One identity queried at rows 3 and 600 (two workgroups), its changes below / above the stored
    one in both orders, then both below: each row has its own verdict, and the store row is lacked
    only if no query reached the stored change. Rows no query names stay Changes, rows at and beyond
    info.rows are 0, the 64 bytes behind max_keys are untouched; the existing fan-out over the view
    with that column returns exactly the model's lacking rows."""
    store, model = held
    k, sub, ch = HELD[10][:3]
    rows = _have(700, seed=5, held_rows=HELD[:10] + HELD[11:150])  # (half of the store is never named)
    rows[3], rows[600] = (k, sub, ch + pair[0], 0, 0, None), (k, sub, ch + pair[1], 0, 0, None)
    wire = _wire(rows)
    wire_t, cols, n = _device_cols(ctx, wire)
    want = _expect(model, wire, cols, n)
    got = _lookup(ctx, store, wire_t, cols, n)
    _check(store, got, want)
    r = model.index[(sub is not None, sub or b"", k)]
    code = {-1: AHEAD, +1: BEHIND}
    assert (got["verdict"][3], got["verdict"][600]) == (code[pair[0]], code[pair[1]])
    assert got["hit"][3] == got["hit"][600] == r
    assert got["lack"][r] == (1 if lacks else 0)
    assert np.all(got["lack"][150:300] == 1) and not got["lack"][300:320].any() and 0 < np.count_nonzero(want["lack"]) < 300
    lacking = [model.rows[j] for j in np.flatnonzero(want["lack"])]
    out_rows, base = store.fanout_rows([None], type_t=got["lack_t"][:store.max_keys])
    assert store._encode_outputs(out_rows, base, store._view(), 1)[0] == _encode(lacking)


# ---- non-queries -------------------------------------------------------------------------------

@pytest.mark.parametrize("spec", [None, {"change_range": (5, 6)}, {"subset": b"s"}, {"key_prefix": b"key-1"}])
def test_non_queries(ctx, held, spec):
    """Blob frames between the Changes, a malformed Change (DRP_F_BAD in the columns) and the rows
    each filter kind excludes are DRP_LOOKUP_NONE with hit_row UINT64_MAX, and are not emitted."""
    store, model = held
    items = _have(200, seed=9)
    wire = b"".join(S.frame(b"blob%d" % j, 2) if j % 6 == 2 else _wire([it]) for j, it in enumerate(items))
    wire_t, cols, n = _device_cols(ctx, wire)
    assert n == 200
    cols = {k: v.clone() for k, v in cols.items()}
    present = [j for j, it in enumerate(items) if j % 6 != 2 and it[0].startswith(b"key-")]
    cols["flags"][present[0]] |= 4
    want = _expect(model, wire, cols, n, spec)
    assert want["verdict"][present[0]] == NONE and not want["verdict"][2::6].any()
    assert 0 < want["counts"][NONE] < n and len(want["out_query"]) > 0
    if spec:
        assert want["counts"][NONE] > _expect(model, wire, cols, n)["counts"][NONE]
    got = _lookup(ctx, store, wire_t, cols, n, spec)
    _check(store, got, want)
    assert np.all(got["hit"][:n][got["verdict"][:n] == NONE] == np.uint64(U64MAX))


def test_wire_ranges(ctx, held):
    """Hand-made columns: a key range that ends one byte past nbytes, a subset range that leaves the
    wire, a payload_off near 2^64 whose sum with key_off wraps (into the wire: the row is the query
    its wrapped range spells, as for drp_latest_device; and past it: no query). nbytes is smaller than
    the tensor, so a read past it stays inside allocated memory and shows as a wrong verdict."""
    import torch
    store, model = held
    rows = [(k, sub, ch, 0, 0, None) for k, sub, ch, *_ in HELD[:13]]
    wire = _wire(rows)
    wire_t, cols, n = _device_cols(ctx, wire)
    q = _host(cols)
    end = lambda i, f: int(q["payload_off"][i]) + int(q[f + "_off"][i]) + int(q[f + "_len"][i])
    nbytes = end(12, "key") - 1             # row 12 (no subset): its key ends one byte past nbytes
    assert HELD[12][1] is None and HELD[10][1] == b"s" and HELD[6][1] == b"s"
    cols = {k: v.clone() for k, v in cols.items()}
    cols["subset_len"][10] = nbytes - int(q["payload_off"][10]) - int(q["subset_off"][10]) + 1  # leaves the wire
    cols["subset_off"][6] = nbytes                                                              # starts at its end
    cols["payload_off"][4] = -1                       # 2^64 - 1: + key_off wraps to key_off - 1, inside the wire
    cols["payload_off"][5] = -int(q["key_off"][5])    # wraps to 0: the wire's first bytes as the key
    cols["payload_off"][8] = -int(q["key_off"][8]) - 1  # 2^64 - 1 after the sum: no wrap of the sum, far outside
    cols["payload_off"][9] = torch.iinfo(torch.int64).min  # 2^63: outside
    want = _expect(model, wire, cols, n, nbytes=nbytes)
    assert [int(want["verdict"][i]) for i in [12, 10, 6, 8, 9]] == [NONE] * 5
    assert want["verdict"][4] == ABSENT and want["verdict"][5] == ABSENT and want["counts"][LEVEL] == 6
    _check(store, _lookup(ctx, store, wire_t[:nbytes], cols, n), want)
    # and with the whole wire rows 12 and 10 are queries again (row 10 with a longer subset: absent)
    want = _expect(model, wire, cols, n)
    assert want["verdict"][12] == LEVEL and want["verdict"][10] == ABSENT
    _check(store, _lookup(ctx, store, wire_t, cols, n), want)


# ---- hash masks ----------------------------------------------------------------------------------

def test_hash_masks(ctx):
    """The hash cut to 0, 1 and 3 bits, set before drp_store_init and held: one probe chain through
    all 300 identities and a byte compare at every step. The outputs are those of the full mask."""
    wire = _wire(_have(400, seed=31))
    outs = []
    try:
        for mask in [U64MAX, 0, 1, 7]:
            ctx.set_latest_hash_mask(mask)
            store, model = _store(ctx, 320, 1 << 15)
            _merge(ctx, store, model, _wire(HELD))
            wire_t, cols, n = _device_cols(ctx, wire)
            got = _lookup(ctx, store, wire_t, cols, n)
            _check(store, got, _expect(model, wire, cols, n))
            outs.append(got)
    finally:
        ctx.set_latest_hash_mask(U64MAX)
    for got in outs[1:]:
        for k in ["verdict", "hit", "counts", "lack", "out_query"]:
            np.testing.assert_array_equal(got[k], outs[0][k], err_msg=k)
        for k in SRC:
            np.testing.assert_array_equal(got["rows"][k], outs[0]["rows"][k], err_msg=k)


# ---- rows_cap ------------------------------------------------------------------------------------

def test_rows_cap(ctx, held):
    """One entry too few: nothing is written to the arrays and *n_out is the true count. Exactly
    enough: complete, the entries behind untouched. rows_cap 0 the same as too few."""
    store, model = held
    wire = _wire(_have(300, seed=12))
    wire_t, cols, n = _device_cols(ctx, wire)
    want = _expect(model, wire, cols, n)
    k = len(want["out_query"])
    assert 1 < k < n
    for cap in [k - 1, k, 0, k + 1]:
        got = _lookup(ctx, store, wire_t, cols, n, rows_cap=cap)
        assert got["n_out"] == k
        _check(store, got, want)


# ---- read-only -----------------------------------------------------------------------------------

def test_read_only(ctx):
    """A lookup with every output requested leaves the columns, the arena, the table and the info
    record byte for byte as they were."""
    store, model = _store(ctx, 320, 1 << 15)
    _merge(ctx, store, model, _wire(HELD))
    _merge(ctx, store, model, _wire([(k, sub, ch + 1, fr, to, b"new") for k, sub, ch, fr, to, _ in HELD[::3]]))
    info, _, _, before = _dump(store)
    wire = _wire(_have(600, seed=13))
    wire_t, cols, n = _device_cols(ctx, wire)
    _check(store, _lookup(ctx, store, wire_t, cols, n), _expect(model, wire, cols, n))
    info2, _, _, after = _dump(store)
    _same_raw(before, after, table=True)
    assert info.as_dict() == info2.as_dict() and info.arena_dead > 0


# ---- after replace and compact -------------------------------------------------------------------

def test_after_replace_and_compact(ctx):
    """Half the rows replaced, then a compact into a fresh arena: the emitted offsets point into the
    new arena and the encoded bytes are the model's."""
    store, model = _store(ctx, 320, 1 << 15)
    _merge(ctx, store, model, _wire(HELD))
    _merge(ctx, store, model, _wire([(k, sub, ch + 2, fr, to, b"replaced-%d" % j)
                                     for j, (k, sub, ch, fr, to, _) in enumerate(HELD[::2])]))
    old = list(model.offs)
    i = store.compact()
    model.compact()
    model.arena_bytes = store.arena_bytes
    assert i.refused == 0 and model.offs != old
    wire = _wire(_have(300, seed=14))
    wire_t, cols, n = _device_cols(ctx, wire)
    want = _expect(model, wire, cols, n)
    assert want["counts"][AHEAD] > want["counts"][BEHIND] > 0  # (the replaced rows lie two above)
    _check(store, _lookup(ctx, store, wire_t, cols, n), want)


# ---- empty store, max_keys = 1 -------------------------------------------------------------------

@pytest.mark.parametrize("max_keys", [1, 64])
def test_empty_store(ctx, max_keys):
    store, model = _store(ctx, max_keys, 256)
    wire = _wire(_have(70, seed=15))
    wire_t, cols, n = _device_cols(ctx, wire)
    want = _expect(model, wire, cols, n)
    assert want["counts"].tolist() == [0, 70, 0, 0, 0] and not want["lack"].any()
    _check(store, _lookup(ctx, store, wire_t, cols, n), want)


def test_one_key_store(ctx):
    """max_keys = 1 (a table of two slots), full: its key is found, every other is absent."""
    store, model = _store(ctx, 1, 256)
    _merge(ctx, store, model, _wire([HELD[0]]))
    wire = _wire(_have(70, seed=16, held_rows=HELD[:2]))
    wire_t, cols, n = _device_cols(ctx, wire)
    want = _expect(model, wire, cols, n)
    assert want["counts"][ABSENT] > 30 and len(want["out_query"]) > 5
    _check(store, _lookup(ctx, store, wire_t, cols, n), want)


# ---- staged --------------------------------------------------------------------------------------

def test_staged(ctx, held):
    """drp_store_lookup_staged over a stream with blobs between the Changes, staged whole and in
    blob-skipping pieces: the mask reply and the DRP_LOOKUP_REPLY_LACK reply are the same bytes in
    every mode, equal to the device path's and to the model's. DRP_E_CAPACITY names the size needed
    and writes nothing; before any stage the call is DRP_E_INVAL."""
    from _gpu import drp_amd
    store, model = held
    with drp_amd.Ctx(0) as fresh:
        st = drp_amd.Store(fresh, 8, 256)
        with pytest.raises(drp_amd.DrpError) as e:
            fresh.store_lookup_staged(st)
        assert e.value.rc == drp_amd.DRP_E_INVAL
    # _blob_stream's keys are key-0 .. key-59 under no subset or "s", changes 0 .. 7: held and not
    big = _blob_stream()
    wire_t, cols, n = _device_cols(ctx, big)
    want = _expect(model, big, cols, n)
    assert all(want["counts"][c] for c in [NONE, ABSENT, BEHIND, LEVEL, AHEAD])
    got = _lookup(ctx, store, wire_t, cols, n)
    _check(store, got, want)
    dev_mask = _rows_wire(store, got)
    dev_lack = store.sync_reply(wire_t, cols, n)
    want_lack = _encode([model.rows[j] for j in np.flatnonzero(want["lack"])])
    assert dev_mask == _encode(want["out_changes"]) and dev_lack == want_lack
    assert 0 < np.count_nonzero(want["lack"]) < 300
    ahead = _encode([model.rows[int(want["hit"][i])] for i in range(n) if want["verdict"][i] == AHEAD])
    try:
        for mode in [drp_amd.BLOB_SKIP_OFF, drp_amd.BLOB_SKIP_ALWAYS]:
            ctx.set_blob_skip(mode)
            ctx.decode_staged(big)
            if mode == drp_amd.BLOB_SKIP_ALWAYS:
                assert ctx.timing().h2d_skipped > 0  # (it was staged in pieces)
            out, rows, counts = ctx.store_lookup_staged(store, reply=drp_amd.LOOKUP_FOUND)
            assert out == dev_mask and rows == len(want["out_query"]) and counts == want["counts"].tolist()
            out, rows, counts = ctx.store_lookup_staged(store, reply=drp_amd.lookup_bit(AHEAD))
            assert out == ahead and rows == want["counts"][AHEAD]
            out, rows, counts = ctx.store_lookup_staged(store, reply=drp_amd.LOOKUP_REPLY_LACK)
            assert out == dev_lack and rows == np.count_nonzero(want["lack"]) and counts == want["counts"].tolist()
            # the capacity contract, and the staged batch still valid behind it
            for reply, whole in [(drp_amd.LOOKUP_FOUND, dev_mask), (drp_amd.LOOKUP_REPLY_LACK, dev_lack)]:
                buf = np.full(len(whole) + 16, AA, np.uint8)
                with pytest.raises(drp_amd.DrpError) as e:
                    ctx.store_lookup_staged(store, reply=reply, cap=len(whole) - 1, out=buf)
                assert e.value.rc == drp_amd.DRP_E_CAPACITY and e.value.written == len(whole)
                assert np.all(buf == AA)
                assert ctx.store_lookup_staged(store, reply=reply, cap=len(whole), out=buf)[0] == whole
        # a filter on the queries: only the have-list's rows under "s" are queries
        out, rows, counts = ctx.store_lookup_staged(store, _filter({"subset": b"s"}), reply=drp_amd.LOOKUP_FOUND)
        sub = _expect(model, big, cols, n, {"subset": b"s"})
        assert out == _encode(sub["out_changes"]) and counts == sub["counts"].tolist() and 0 < rows < len(want["out_query"])
    finally:
        ctx.set_blob_skip(drp_amd.BLOB_SKIP_OFF)


# ---- Python --------------------------------------------------------------------------------------

def test_store_get(ctx, held):
    """Store.get over 100 keys: 40 the store does not hold, one twice, one under a subset."""
    store, model = held
    rng = random.Random(21)
    plain = [h for h in HELD if h[1] is None]
    keys = [h[0] for h in rng.sample(plain, 58)]
    keys.append(keys[5])                       # twice
    keys.append((HELD[2][1], HELD[2][0]))      # (subset, key)
    keys += [b"nokey-%d" % j for j in range(38)] + [HELD[2][0], (b"zz", plain[0][0])]  # (held only under "s"; and not under "zz")
    rng.shuffle(keys)
    assert len(keys) == 100
    ident = lambda k: (True, k[0], k[1]) if isinstance(k, tuple) else (False, b"", k)
    want_rows = [model.index.get(ident(k), -1) for k in keys]
    assert want_rows.count(-1) == 40
    hit, wire = store.get(keys)
    assert hit.dtype == np.int64 and hit.tolist() == want_rows
    assert wire == _encode([model.rows[r] for r in want_rows if r >= 0])
    hit, wire = store.get([])
    assert len(hit) == 0 and wire == b""


# ---- end to end ----------------------------------------------------------------------------------

def _content(k, sub, ch):
    """A Change whose content follows from its identity and change: two stores that hold an identity
    at one change hold the same row (a content comparison at equal change is out of scope)."""
    return (k, sub, ch, ch % 128, (ch * 7) % 128, b"%s@%d" % (k, ch) if ch % 3 else None)


def _have_list(model):
    return _wire([(c.key, c.subset if c.has else None, c.change, c.frm, c.to, None) for c in model.rows])


def test_end_to_end(ctx):
    """Two stores from overlapping pools, neither containing the other. B's have-list (its rows
    without values) to A.sync_reply, the reply merged into B; the same the other way round. Then the
    two digests are equal and a second sync_reply in each direction is empty."""
    import torch
    rng = random.Random(41)
    mk = lambda lo, hi: [_content(b"key-%d" % rng.randrange(lo, hi), rng.choice([None, None, b"s"]), rng.randrange(1, 9))
                         for _ in range(600)]
    A, ma = _store(ctx, 1024, 1 << 16)
    B, mb = _store(ctx, 1024, 1 << 16)
    _merge(ctx, A, ma, _wire(mk(0, 200)))
    _merge(ctx, B, mb, _wire(mk(100, 300)))
    ia, ib = set(ma.index), set(mb.index)
    assert ia - ib and ib - ia and ia & ib
    assert not torch.equal(A.digest(8).cpu(), B.digest(8).cpu())

    def lacking(src, have):
        """src's rows the holder of `have` lacks: not held, or held at a smaller change."""
        return [c for c in src.rows if (c.has, c.subset, c.key) not in have.index or
                have.rows[have.index[(c.has, c.subset, c.key)]].change < c.change]

    for src, ms, dst, md in [(A, ma, B, mb), (B, mb, A, ma)]:
        want = _encode(lacking(ms, md))
        wire_t, cols, n = _device_cols(ctx, _have_list(md))
        reply = src.sync_reply(wire_t, cols, n)
        assert reply == want and reply
        _merge(ctx, dst, md, reply)
    assert {(c.has, c.subset, c.key): c for c in ma.rows} == {(c.has, c.subset, c.key): c for c in mb.rows}
    assert torch.equal(A.digest(8).cpu(), B.digest(8).cpu())
    for src, md in [(A, mb), (B, ma)]:
        wire_t, cols, n = _device_cols(ctx, _have_list(md))
        assert src.sync_reply(wire_t, cols, n) == b""
    # under a filter the reply is the lacking rows the filter keeps
    _, nothing = _store(ctx, 64, 1 << 12)
    wire_t, cols, n = _device_cols(ctx, _have_list(nothing))
    assert n == 0
    assert A.sync_reply(wire_t, cols, n, _filter({"subset": b"s"})) == _encode([c for c in ma.rows if c.has])
