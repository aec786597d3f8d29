"""GPU parity for the digest calls (drp_digest_device, drp_digest_diff_device,
drp_select_buckets_device, Store.digest, Store.reconcile). Every comparison is exact, against an
expected side built here on the CPU from the oracle's decode, python-xxhash and the formulas of
include/drp.h "digest / reconcile":
    merge(a, v) = (a ^ (rotl(v * P2, 31) * P1)) * P1 + P4
    ident = XXH64(key) [merge XXH64(subset)]; fp = avalanche(merge over change, from, to, flags & 3
    [, XXH64(value)]); bucket = ident >> (64 - bits); cell = (rows, sum of fp), all modulo 2^64.
The device columns are the oracle's, uploaded (the decode tests show the device's are the same)."""
import random

import numpy as np
import pytest
import xxhash

import _oracle as O
import _streams as S
from _relay import (SRC_KEYS, Change, change_at as _change, make_filter as _filter, mask as _mask, rows as _rows,
                    wire_winners as _winners)
from test_gpu_store import _merge, _store, _wire

pytestmark = pytest.mark.gpu

M64 = 2**64 - 1
P1, P2, P3, P4 = 11400714785074694791, 14029467366897019727, 1609587929392839161, 9650029242287828579
# (255 .. 257: either side of the length from which four lanes hash a value, DIG_QUAD_MIN of drp_digest.hip)
VALUE_LENS = [None, 0, 1, 3, 4, 7, 8, 31, 32, 33, 63, 64, 65, 255, 256, 257, 4101]
KEY_LENS = [0, 1, 8, 32, 40]
SUBSETS = [None, b"", b"abcde"]
N_BIG = 5000


@pytest.fixture(scope="module")
def ctx():
    from _gpu import drp_amd
    c = drp_amd.Ctx(0)
    c.set_blob_skip(drp_amd.BLOB_SKIP_OFF)
    yield c
    c.close()


def _lds_bits():
    from _gpu import drp_amd
    return drp_amd.DIGEST_LDS_BITS


# ---- the expected side ---------------------------------------------------------------------

def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & M64


def _merge_h(a, v):
    return ((a ^ (_rotl((v * P2) & M64, 31) * P1 & M64)) * P1 + P4) & M64


def _ident(c):
    h = xxhash.xxh64_intdigest(c.key)
    return _merge_h(h, xxhash.xxh64_intdigest(c.subset)) if c.has else h


def _fp(c, ident):
    h = ident
    for v in (c.change, c.frm, c.to, (1 if c.has else 0) | (2 if c.hv else 0)):
        h = _merge_h(h, v)
    if c.hv:
        h = _merge_h(h, xxhash.xxh64_intdigest(c.value))
    h ^= h >> 33
    h = h * P2 & M64
    h ^= h >> 29
    h = h * P3 & M64
    return h ^ (h >> 32)


def _hashes(changes):
    """ident and fp of every Change, as uint64 arrays."""
    ids = [_ident(c) for c in changes]
    return np.array(ids, np.uint64), np.array([_fp(c, i) for c, i in zip(changes, ids)], np.uint64)


def _buckets(ident, bits):
    return (ident >> np.uint64(64 - bits)).astype(np.int64) if bits else np.zeros(len(ident), np.int64)


def _cells(ident, fp, bits):
    """The expected cells of the rows with these hashes: a (2**bits, 2) uint64 array."""
    cells = np.zeros((1 << bits, 2), np.uint64)
    b = _buckets(ident, bits)
    np.add.at(cells[:, 0], b, np.uint64(1))
    np.add.at(cells[:, 1], b, fp)  # (wraps modulo 2^64)
    return cells


def _cells_of(changes, bits):
    return _cells(*_hashes(changes), bits)


class Batch:
    """A wire, the oracle's rows of it, and per row the identity hash and the fingerprint (0 for a row
    that is no well-formed Change). bad: rows marked DRP_F_BAD in the columns, as the decoder marks a
    malformed Change."""

    def __init__(self, wire, bad=()):
        self.wire = wire
        self.w = np.frombuffer(wire, np.uint8)
        ref = O.decode_batch(wire)
        assert ref["err_code"] == 0
        self.n = ref["nframes"]
        self.ref = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in ref.items()}
        for i in bad:
            assert self.ref["type"][i] == 1
            self.ref["flags"][i] |= 4
        self.ok = _mask(self.w, self.ref, self.n, {})
        self.ident, self.fp = np.zeros(self.n, np.uint64), np.zeros(self.n, np.uint64)
        idx = np.flatnonzero(self.ok)
        self.ident[idx], self.fp[idx] = _hashes([_change(wire, self.ref, int(i)) for i in idx])
        self._dev = None

    def device(self):
        """(wire_t, cols) on the device, uploaded once and read only."""
        import torch
        if self._dev is None:
            dev = torch.device("cuda", 0)
            signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.uint8): np.uint8}
            cols = {}
            for k in ["payload_off", "payload_len", "type", "flags"] + O.COLS32 + O.COLS64:
                a = np.zeros(max(self.n, 1), self.ref[k].dtype)
                a[:self.n] = self.ref[k][:self.n]
                cols[k] = torch.from_numpy(a.view(signed[a.dtype])).to(dev)
            self._dev = torch.from_numpy(self.w.copy()).to(dev), cols
        return self._dev

    def ends(self):
        """Per row the end of its last byte range (key, subset if present, value if present)."""
        r, n = self.ref, self.n
        po = r["payload_off"][:n].astype(np.int64)
        e = po + r["key_off"][:n] + r["key_len"][:n]
        e = np.maximum(e, np.where(r["flags"][:n] & 1, po + r["subset_off"][:n] + r["subset_len"][:n], 0))
        return np.maximum(e, np.where(r["flags"][:n] & 2, po + r["value_off"][:n] + r["value_len"][:n], 0))

    def candidates(self, n=None, spec=None, nbytes=None):
        """(candidate rows, selected rows left out for a range outside the wire) among rows [0, n)."""
        n = self.n if n is None else n
        sel = _mask(self.w, self.ref, n, spec or {})
        inside = self.ends()[:n] <= (len(self.wire) if nbytes is None else nbytes)
        return np.flatnonzero(sel & inside), np.flatnonzero(sel & ~inside)

    def cells(self, idx, bits):
        return _cells(self.ident[idx], self.fp[idx], bits)


def _digest(ctx, batch, bits, n=None, spec=None, nbytes=None):
    """drp_digest_device into poisoned outputs: (cells as (2**bits, 2) uint64, totals)."""
    import torch
    wire_t, cols = batch.device()
    cells = torch.full((1 << bits, 2), -1, dtype=torch.int64, device=wire_t.device)
    tot = torch.full((2,), -1, dtype=torch.int64, device=wire_t.device)
    ctx.digest_device(wire_t if nbytes is None else wire_t[:nbytes], cols, batch.n if n is None else n, _filter(spec),
                      bits, cells, tot)
    torch.cuda.synchronize()
    return cells.cpu().numpy().view(np.uint64), [int(v) for v in tot.cpu()]


def _check_digest(ctx, batch, bits, n=None, spec=None, nbytes=None):
    idx, out = batch.candidates(n, spec, nbytes)
    got, tot = _digest(ctx, batch, bits, n, spec, nbytes)
    np.testing.assert_array_equal(got, batch.cells(idx, bits), err_msg=f"bits {bits} n {n} {spec}")
    assert tot == [len(idx), len(out)]
    return idx, out


def _select_buckets(ctx, batch, bits, bset, n=None, spec=None, nbytes=None):
    """drp_select_buckets_device with the bucket set `bset` (uint64 words): (rows, sel_idx)."""
    import torch
    wire_t, cols = batch.device()
    n = batch.n if n is None else n
    dev = wire_t.device
    rows = {k: torch.full((max(n, 1),), 0x55, dtype=(torch.int32 if k.endswith("_len") else
                                                     torch.uint8 if k == "flags" else torch.int64), device=dev)
            for k in SRC_KEYS}
    idx_t = torch.full((max(n, 1),), -1, dtype=torch.int64, device=dev)
    nsel_t = torch.full((1,), -1, dtype=torch.int64, device=dev)
    bset_t = torch.from_numpy(np.asarray(bset, np.uint64).view(np.int64).copy()).to(dev)
    ctx.select_buckets_device(wire_t if nbytes is None else wire_t[:nbytes], cols, n, _filter(spec), bits, bset_t, rows,
                              idx_t, nsel_t)
    torch.cuda.synchronize()
    nsel = int(nsel_t.cpu()[0])
    assert np.all(idx_t.cpu().numpy()[nsel:] == -1)
    return {k: v.cpu().numpy()[:nsel] for k, v in rows.items()}, idx_t.cpu().numpy()[:nsel]


def _check_rows(batch, got, idx, want_idx, what=""):
    np.testing.assert_array_equal(idx, want_idx, err_msg=str(what))
    want = _rows(batch.ref, want_idx)
    for k in SRC_KEYS:
        np.testing.assert_array_equal(got[k].astype(want[k].dtype), want[k], err_msg=f"{what} {k}")


def _set_words(buckets, bits):
    w = np.zeros(max(1, (1 << bits) // 64), np.uint64)
    for b in buckets:
        w[b >> 6] |= np.uint64(1 << (b & 63))
    return w


def _diff(ctx, a, b, bits):
    """drp_digest_diff_device of two (2**bits, 2) uint64 arrays: (set words as uint64, n_diff)."""
    import torch
    dev = torch.device("cuda", 0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int64).copy()).to(dev)
    bset = torch.full((max(1, (1 << bits) // 64),), -1, dtype=torch.int64, device=dev)
    nd = torch.full((1,), -1, dtype=torch.int64, device=dev)
    ctx.digest_diff_device(up(a), up(b), bits, bset, nd)
    torch.cuda.synchronize()
    return bset.cpu().numpy().view(np.uint64), int(nd.cpu()[0])


# ---- the shared batch ------------------------------------------------------------------------

def _big_wire():
    """N_BIG frames: Changes that run through every (value length, key length, subset) of the lists
    above, a blob frame after every 50th. change = i % 9 + 1; keys start with "k<i % 1000>-"."""
    rng = random.Random(17)
    combos = [(v, k, s) for v in VALUE_LENS for k in KEY_LENS for s in SUBSETS]
    rng.shuffle(combos)
    parts = []
    for i in range(N_BIG):
        if i % 50 == 49:
            parts.append(S.frame(rng.randbytes(rng.randrange(0, 40)), 2))
            continue
        vl, kl, sub = combos[i % len(combos)]
        key = (b"k%d-" % (i % 1000) + rng.randbytes(40))[:kl]
        parts.append(S.frame(S.change_payload(key, i % 9 + 1, rng.randrange(128), rng.randrange(1 << 40),
                                              value=None if vl is None else rng.randbytes(vl), subset=sub)))
    return b"".join(parts)


@pytest.fixture(scope="module")
def big():
    """The shared batch (read only): row 2500 is marked malformed."""
    b = Batch(_big_wire(), bad=[2500])
    assert b.n == N_BIG and int(b.ok.sum()) == N_BIG - N_BIG // 50 - 1
    return b


def test_the_expected_side_is_xxh64():
    """The formulas' constants against python-xxhash: XXH64 of 32 zero bytes is built from P1 .. P4."""
    v = [(P1 + P2) & M64, P2, 0, (0 - P1) & M64]
    v = [_rotl(x, 31) * P1 & M64 for x in v]  # (one stripe of zeros: acc + 0 * P2)
    h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & M64
    for x in v:
        h = _merge_h(h, x)
    h = (h + 32) & M64
    h ^= h >> 33
    h = h * P2 & M64
    h ^= h >> 29
    h = h * P3 & M64
    assert h ^ (h >> 32) == xxhash.xxh64_intdigest(bytes(32))


# ---- hash branches and row counts ------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 4096, 4097, N_BIG])
def test_hash_branches_and_row_counts(ctx, big, n):
    """Rows [0, n) of the shared batch: the wave (64) and workgroup (1024 rows) sizes, one below, at
    and above, and several workgroups; every tail of XXH64 in keys, subsets and values, blobs and the malformed
    row in between. In LDS (bits 4) and in global memory (above the threshold)."""
    for bits in [4, _lds_bits() + 1]:
        idx, out = _check_digest(ctx, big, bits, n)
        assert len(out) == 0 and len(idx) == int(big.ok[:n].sum())
    if n == N_BIG:  # the shared batch holds every combination
        seen = {(None if not f & 2 else int(v), int(k), None if not f & 1 else int(s))
                for f, v, k, s in zip(big.ref["flags"][big.ok], big.ref["value_len"][big.ok], big.ref["key_len"][big.ok],
                                      big.ref["subset_len"][big.ok])}
        assert seen == {(v, k, None if s is None else len(s)) for v in VALUE_LENS for k in KEY_LENS for s in SUBSETS}


def test_wide_values(ctx):
    """Values that four lanes hash together, sixteen rows a round: a wave with one such row, waves
    with 13 and with 51 (more than one round, the last not full), a wave of 64 (four full rounds), and
    lengths that leave every tail (0 .. 31 bytes behind the last stripe)."""
    rng = random.Random(29)
    wide = lambda i: i == 5 or (64 <= i < 128 and i % 5 == 0) or (128 <= i < 192 and i % 5) or 192 <= i < 256
    rows = [(b"key-%d" % i, None, i % 7, 1, 2, rng.randbytes(256 + (i * 53) % 1000 if wide(i) else i % 200))
            for i in range(300)]
    b = Batch(_wire(rows))
    vl = b.ref["value_len"][:256].reshape(4, 64)
    assert [int((w >= 256).sum()) for w in vl] == [1, 13, 51, 64]
    assert {int(v) % 32 for v in b.ref["value_len"][:300] if v >= 256} == set(range(32))
    for bits in [2, 14]:
        _check_digest(ctx, b, bits)


def _np_merge(a, v):
    """merge over uint64 arrays (numpy wraps modulo 2^64)."""
    t = v * np.uint64(P2)
    t = ((t << np.uint64(31)) | (t >> np.uint64(33))) * np.uint64(P1)
    return (a ^ t) * np.uint64(P1) + np.uint64(P4)


def test_several_chunks_per_workgroup(ctx):
    """From 2 * 128 * 1024 rows on a dig_cells workgroup takes more than one chunk of 1024 rows
    (DIG_CHUNKS, DIG_GRID_MIN of drp_kernels.h). 270,001 Changes of the C2 shape (10-digit keys, 64
    value bytes, no subset); the expected side hashes keys and values with python-xxhash and merges
    in numpy. In LDS and in global memory."""
    import torch
    n = 270_001
    w = S.c2_stream(n, seed=5)
    ref = O.decode_batch(w.tobytes())
    assert ref["nframes"] == n and ref["err_code"] == 0 and np.all(ref["flags"][:n] == 2)
    mv = memoryview(w.tobytes())
    ko = (ref["payload_off"][:n] + ref["key_off"][:n]).tolist()
    vo = (ref["payload_off"][:n] + ref["value_off"][:n]).tolist()
    ident = np.array([xxhash.xxh64_intdigest(mv[o:o + 10]) for o in ko], np.uint64)
    vh = np.array([xxhash.xxh64_intdigest(mv[o:o + 64]) for o in vo], np.uint64)
    assert np.all(ref["key_len"][:n] == 10) and np.all(ref["value_len"][:n] == 64)
    h = ident
    for v in (ref["change"][:n], ref["from"][:n], ref["to"][:n], np.full(n, 2, np.uint64), vh):
        h = _np_merge(h, v.astype(np.uint64))
    h ^= h >> np.uint64(33)
    h *= np.uint64(P2)
    h ^= h >> np.uint64(29)
    h *= np.uint64(P3)
    h ^= h >> np.uint64(32)
    assert int(h[7]) == _fp(_change(mv, ref, 7), int(ident[7]))  # (the numpy form is the scalar one)
    dev = torch.device("cuda", 0)
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.uint8): np.uint8}
    cols = {k: torch.from_numpy(ref[k][:n].view(signed[ref[k].dtype])).to(dev)
            for k in ["payload_off", "payload_len", "type", "flags"] + O.COLS32 + O.COLS64}
    wire_t = torch.from_numpy(w).to(dev)
    for bits in [5, _lds_bits() + 2]:
        cells = torch.full((1 << bits, 2), -1, dtype=torch.int64, device=dev)
        tot = torch.full((2,), -1, dtype=torch.int64, device=dev)
        ctx.digest_device(wire_t, cols, n, None, bits, cells, tot)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(cells.cpu().numpy().view(np.uint64), _cells(ident, h, bits))
        assert [int(v) for v in tot.cpu()] == [n, 0]


def test_no_rows(ctx, big):
    """n = 0: the cells and totals are zeroed, nothing else happens."""
    got, tot = _digest(ctx, big, 3, n=0)
    assert not got.any() and tot == [0, 0]


@pytest.mark.parametrize("bits", ["0", "5", "6", "7", "lds", "lds+1", "16"])
def test_bits(ctx, big, bits):
    """One cell that every row contends for; either side of one bitmap word; the last size summed in
    LDS and the first summed in global memory; the most."""
    bits = {"lds": _lds_bits(), "lds+1": _lds_bits() + 1}.get(bits) or int(bits)
    idx, _ = _check_digest(ctx, big, bits)
    if bits == 0:
        got, _ = _digest(ctx, big, 0)
        assert int(got[0, 0]) == len(idx) and int(got[0, 1]) == int(big.fp[idx].sum(dtype=np.uint64))


@pytest.mark.parametrize("spec", [{"change_range": (3, 5)}, {"key_prefix": b"k1"}, {"subset": b"abcde"},
                                  {"subset": b""}, {"subset_none": True}])
def test_filters(ctx, big, spec):
    idx, _ = _check_digest(ctx, big, 7, spec=spec)
    assert 50 < len(idx) < int(big.ok.sum()) - 50


# ---- wire bounds -----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small():
    """130 Changes, every one with a value (the model of test_gpu_relay_wire_bounds)."""
    return Batch(b"".join(S.frame(S.change_payload(b"key%04d" % i, i % 7 + 1, 1, 2, value=b"value%d" % i,
                                                   subset=b"ab" if i % 2 else None)) for i in range(130)))


@pytest.mark.parametrize("where", ["value", "key"])
def test_wire_bounds(ctx, small, where):
    """nbytes cut inside the last row's value, and inside its key (the value lies behind it): the row
    is not read, it is counted in totals[1], the cells hold the other rows; the bucket select with
    every bucket set keeps exactly those. A cut right behind the row leaves nothing out."""
    r, last = small.ref, small.n - 1
    at = int(r["payload_off"][last]) + int(r[where + "_off"][last])
    for bits in [0, 6, _lds_bits() + 1]:
        idx, out = _check_digest(ctx, small, bits, nbytes=at + 2)
        assert list(out) == [last] and len(idx) == last
    got, sel = _select_buckets(ctx, small, 6, _set_words(range(64), 6), nbytes=at + 2)
    _check_rows(small, got, sel, np.arange(last), where)
    end = int(small.ends()[last])
    assert end == len(small.wire)
    idx, out = _check_digest(ctx, small, 6, nbytes=end)
    assert len(out) == 0 and len(idx) == small.n
    idx, out = _check_digest(ctx, small, 6, nbytes=end - 1)
    assert list(out) == [last]
    if where == "value":  # a byte condition that still fits: the select keeps the row, the digest leaves it out
        idx, out = _check_digest(ctx, small, 6, spec={"key_prefix": b"key"}, nbytes=at + 2)
        assert list(out) == [last]


# ---- multiset, order, hash mask ----------------------------------------------------------------

def _small_rows(n, seed):
    rng = random.Random(seed)
    return [(b"key-%d" % i, rng.choice([None, b"", b"s"]), rng.randrange(1, 9), i % 128, (i * 7) % 128,
             rng.randbytes(rng.randrange(0, 70)) if i % 4 else None) for i in range(n)]


def test_multiset_and_order(ctx):
    """A row that occurs twice counts twice; the same rows in another order give the same cells."""
    rows = _small_rows(300, 3)
    twice = Batch(_wire(rows + [rows[41]]))
    idx, _ = _check_digest(ctx, twice, 16)
    got, _ = _digest(ctx, twice, 16)
    b = int(twice.ident[41] >> np.uint64(48))
    assert int(got[b, 0]) == 2 and int(got[b, 1]) == (2 * int(twice.fp[41])) & M64
    assert int(got[:, 0].sum()) == 301
    perm = rows + [rows[41]]
    random.Random(9).shuffle(perm)
    other = Batch(_wire(perm))
    for bits in [0, 8, 16]:
        a, _ = _digest(ctx, twice, bits)
        c, _ = _digest(ctx, other, bits)
        np.testing.assert_array_equal(a, c)


def test_hash_mask_does_not_reach_the_digest(ctx, big):
    """drp_set_latest_hash_mask is a hook of the grouping tables: the cells and the bucket select are
    the same with mask 0 and with all ones."""
    want = {bits: big.cells(big.candidates()[0], bits) for bits in [6, 16]}
    hand = _set_words([1, 40, 63], 6)
    try:
        for mask in [0, M64]:
            ctx.set_latest_hash_mask(mask)
            for bits in [6, 16]:
                np.testing.assert_array_equal(_digest(ctx, big, bits)[0], want[bits])
            _, sel = _select_buckets(ctx, big, 6, hand)
            idx = big.candidates()[0]
            np.testing.assert_array_equal(sel, idx[np.isin(_buckets(big.ident[idx], 6), [1, 40, 63])])
    finally:
        ctx.set_latest_hash_mask(M64)


# ---- diff and bucket select --------------------------------------------------------------------

def test_diff(ctx, big):
    """Equal cells: the empty set. Every cell altered: every bit, and none beyond 2^bits in the one
    word of bits < 6. A few cells altered in count or in sum only: exactly those."""
    for bits in [0, 3, 5, 6, 7, 16]:
        a = big.cells(big.candidates()[0], bits)
        bset, nd = _diff(ctx, a, a, bits)
        assert nd == 0 and not bset.any()
        b = a.copy()
        b[:, 0] += np.uint64(1)
        bset, nd = _diff(ctx, a, b, bits)
        assert nd == 1 << bits
        np.testing.assert_array_equal(bset, _set_words(range(1 << bits), bits))
        rng = random.Random(bits)
        pick = sorted(rng.sample(range(1 << bits), min(1 << bits, 5)))
        b = a.copy()
        for j, p in enumerate(pick):
            b[p, j % 2] ^= np.uint64(1 << 63)
        bset, nd = _diff(ctx, b, a, bits)
        assert nd == len(pick)
        np.testing.assert_array_equal(bset, _set_words(pick, bits))


def test_bucket_select(ctx, big):
    """No bucket set: no rows. Every bucket set: drp_select_device's rows (all ranges are inside the
    wire). A hand-made set, with and without a filter: the candidates of those buckets in row order,
    with their sel_idx; rows [0, n) only."""
    import torch
    idx, _ = big.candidates()
    got, sel = _select_buckets(ctx, big, 7, _set_words([], 7))
    assert len(sel) == 0
    got, sel = _select_buckets(ctx, big, 7, _set_words(range(128), 7))
    _check_rows(big, got, sel, idx, "all")
    wire_t, cols = big.device()
    rows = {k: torch.zeros(big.n, dtype=(torch.int32 if k.endswith("_len") else torch.uint8 if k == "flags" else
                                         torch.int64), device=wire_t.device) for k in SRC_KEYS}
    idx_t = torch.zeros(big.n, dtype=torch.int64, device=wire_t.device)
    nsel_t = torch.zeros(1, dtype=torch.int64, device=wire_t.device)
    ctx.select_device(wire_t, cols, big.n, None, rows, idx_t, nsel_t)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(idx_t.cpu().numpy()[:int(nsel_t.cpu()[0])], sel)
    for k in SRC_KEYS:
        np.testing.assert_array_equal(rows[k].cpu().numpy()[:len(sel)], got[k], err_msg=k)
    for bits, hand in [(7, [3, 64, 127]), (0, [0]), (5, [0, 31]), (16, list(range(0, 65536, 7)))]:
        for spec, n in [(None, None), ({"change_range": (2, 6)}, None), (None, 1025)]:
            cand, _ = big.candidates(n, spec)
            want = cand[np.isin(_buckets(big.ident[cand], bits), hand)]
            got, sel = _select_buckets(ctx, big, bits, _set_words(hand, bits), n, spec)
            _check_rows(big, got, sel, want, (bits, spec, n))
            assert bits == 0 or 0 < len(want) < len(cand)


def test_invalid_arguments(ctx, big):
    import ctypes as C
    import torch
    from _gpu import drp_amd
    wire_t, cols = big.device()
    z = torch.zeros(2 << 16, dtype=torch.int64, device=wire_t.device)
    rows = {k: torch.zeros(big.n, dtype=(torch.int32 if k.endswith("_len") else torch.uint8 if k == "flags" else
                                         torch.int64), device=wire_t.device) for k in SRC_KEYS}
    with pytest.raises(drp_amd.DrpError) as e:
        ctx.digest_device(wire_t, cols, big.n, None, 17, z)
    assert e.value.rc == drp_amd.DRP_E_INVAL
    with pytest.raises(drp_amd.DrpError) as e:
        ctx.digest_device(wire_t, cols, big.n, None, 4, None)
    assert e.value.rc == drp_amd.DRP_E_INVAL
    with pytest.raises(drp_amd.DrpError) as e:
        ctx.digest_device(wire_t, cols, big.n, drp_amd.make_filter(flags=0x40), 4, z)
    assert e.value.rc == drp_amd.DRP_E_INVAL
    with pytest.raises(drp_amd.DrpError) as e:
        ctx.digest_diff_device(z, z, 17, z, z)
    assert e.value.rc == drp_amd.DRP_E_INVAL
    for bits, bset in [(17, z), (4, None)]:
        with pytest.raises(drp_amd.DrpError) as e:
            ctx.select_buckets_device(wire_t, cols, big.n, None, bits, bset, rows, None, z)
        assert e.value.rc == drp_amd.DRP_E_INVAL
    assert C.sizeof(drp_amd.DigestCell) == 16


# ---- store -------------------------------------------------------------------------------------

def _content(key, sub, change):
    """A Change whose content is a function of (identity, change)."""
    h = xxhash.xxh64_intdigest(key + b"/" + (sub or b"-") + b"/%d" % change)
    return (key, sub, change, h % 128, (h >> 8) % 128, None if h % 5 == 0 else (b"%x" % h) * (1 + h % 4))


def test_store(ctx):
    """Three overlapping batches merged: the store's digest over n = max_keys is the expected digest
    of the model's rows, unchanged by a compact; after a merge that replaces k rows only the buckets
    of those identities differ."""
    rng = random.Random(23)
    idents = [(b"key-%d" % i, rng.choice([None, b"", b"s"])) for i in range(900)]
    store, model = _store(ctx, 1000, 1 << 18)
    for lo, hi in [(0, 500), (300, 800), (100, 900)]:
        _merge(ctx, store, model, _wire([_content(k, s, rng.randrange(1, 6)) for k, s in idents[lo:hi]]))
    assert model.seen["replaced_gt"] and model.seen["stale"] and len(model.rows) == 900 and model.dead
    bits = 12
    want = _cells_of(model.rows, bits)
    got = store.digest(bits).cpu().numpy().view(np.uint64)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(store.digest(bits, n=len(model.rows)).cpu().numpy().view(np.uint64), want)
    np.testing.assert_array_equal(store.digest(3).cpu().numpy().view(np.uint64), _cells_of(model.rows, 3))
    flt = {"subset": b"s"}
    np.testing.assert_array_equal(store.digest(bits, _filter(flt)).cpu().numpy().view(np.uint64),
                                  _cells_of([c for c in model.rows if c.has and c.subset == b"s"], bits))
    assert store.compact(1 << 18).refused == 0  # (room for the merge below)
    model.compact()
    np.testing.assert_array_equal(store.digest(bits).cpu().numpy().view(np.uint64), want)
    k = 7
    picked = rng.sample(range(900), k)
    _, cnt = _merge(ctx, store, model, _wire([_content(*idents[i], 9) for i in picked]))
    assert cnt["replaced"] == k
    after = store.digest(bits).cpu().numpy().view(np.uint64)
    np.testing.assert_array_equal(after, _cells_of(model.rows, bits))
    changed = np.flatnonzero((after != want).any(axis=1))
    touched = {int(b) for b in _buckets(_hashes([c for c in model.rows if c.change == 9])[0], bits)}
    assert set(changed.tolist()) == touched and 0 < len(touched) <= k
    bset, nd = _diff(ctx, want, after, bits)
    assert nd == len(touched)
    np.testing.assert_array_equal(bset, _set_words(touched, bits))


def test_end_to_end(ctx):
    """Two stores of about 2000 identities that differ in 5: 2 only in A, 1 only in B, 2 with a
    greater change in A. Each side's reconcile against the other's digest (both computed before either
    merge) is exactly its rows in the differing buckets, in store order; after each merges the other's
    bytes both digests are equal, and equal to the digest of the latest per key over the union."""
    rng = random.Random(31)
    bits = 8
    idents = [(b"key-%d" % i, rng.choice([None, None, b"s", b""])) for i in range(2003)]
    base = [_content(k, s, rng.randrange(1, 50)) for k, s in idents[:2000]]
    rng.shuffle(base)
    rows_a = base + [_content(*idents[2000], 5), _content(*idents[2001], 6)]
    rows_a += [_content(k, s, ch + 3) for k, s, ch, *_ in base[10:12]]
    rows_b = base[::-1] + [_content(*idents[2002], 7)]
    A, ma = _store(ctx, 2100, 1 << 18)
    B, mb = _store(ctx, 2100, 1 << 18)
    _merge(ctx, A, ma, _wire(rows_a))
    _merge(ctx, B, mb, _wire(rows_b))
    assert len(ma.rows) == 2002 and len(mb.rows) == 2001
    ca, cb = _cells_of(ma.rows, bits), _cells_of(mb.rows, bits)
    differ = np.flatnonzero((ca != cb).any(axis=1))
    assert 3 <= len(differ) <= 5
    da, db = A.digest(bits), B.digest(bits)
    np.testing.assert_array_equal(da.cpu().numpy().view(np.uint64), ca)
    np.testing.assert_array_equal(db.cpu().numpy().view(np.uint64), cb)
    wire_a, buckets_a = A.reconcile(db, bits)
    wire_b, buckets_b = B.reconcile(da.cpu().numpy(), bits)  # (a numpy array as well as a tensor)
    np.testing.assert_array_equal(buckets_a, differ)
    np.testing.assert_array_equal(buckets_b, differ)
    for wire, model in [(wire_a, ma), (wire_b, mb)]:
        ref = O.decode_batch(wire)
        assert ref["err_code"] == 0 and ref["consumed"] == len(wire)
        got = [_change(wire, ref, i) for i in range(ref["nframes"])]
        want = [c for c in model.rows if int(_buckets(np.array([_ident(c)], np.uint64), bits)[0]) in set(differ.tolist())]
        assert got == want and len(want) < 100
    sent_a, sent_b = O.decode_batch(wire_a)["nframes"], O.decode_batch(wire_b)["nframes"]
    assert sent_a == sent_b + 1  # (the 2 only in A against the 1 only in B)
    _, cnt = _merge(ctx, B, mb, wire_a)
    assert (cnt["inserted"], cnt["replaced"], cnt["stale"], cnt["unchanged"]) == (2, 2, 0, sent_a - 4)
    _, cnt = _merge(ctx, A, ma, wire_b)
    assert (cnt["inserted"], cnt["replaced"], cnt["stale"], cnt["unchanged"]) == (1, 0, 2, sent_b - 3)
    union = _cells_of(_winners(_wire(rows_a + rows_b))[1], bits)
    np.testing.assert_array_equal(A.digest(bits).cpu().numpy().view(np.uint64), union)
    np.testing.assert_array_equal(B.digest(bits).cpu().numpy().view(np.uint64), union)
    # a reconcile of equal stores sends nothing
    wire, buckets = A.reconcile(B.digest(bits), bits)
    assert wire == b"" and len(buckets) == 0
