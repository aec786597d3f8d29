"""GPU parity for the refined digest calls (drp_digest_refine_device, drp_digest_diff_cells_device,
drp_select_refined_device, Store.digest_refined, Store.reconcile_refined). Every comparison is exact,
against a numpy model built from the formulas of include/drp.h "refined digests":
    slot(b)    = the set bits of bucket_set below bit b
    sub(row)   = (ident >> (64 - bits - sub_bits)) & (2^sub_bits - 1)
    cell2(row) = slot(bucket(row)) * 2^sub_bits + sub(row);  cells2[c] = (rows, sum of fp) modulo 2^64
ident, fp and the candidates are test_gpu_digest's expected side (the oracle's decode, python-xxhash).
Outputs are poisoned before every call; cells2 carries a sentinel, so "left untouched" is checked."""
import random

import numpy as np
import pytest
import xxhash

import _oracle as O
import _streams as S
from _relay import SRC_KEYS, change_at as _change, make_filter as _filter, wire_winners as _winners
from test_gpu_digest import (M64, P2, P3, _buckets, _cells_of, _check_rows, _content, _diff, _digest, _fp,
                             _hashes, _np_merge, _set_words, big, ctx)  # noqa: F401 (big, ctx: fixtures)
from test_gpu_store import _merge, _store, _wire

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A5A5A5A5A
LDS_CELLS = 1024  # csrc/drp_kernels.h DIG_REFINE_LDS_CELLS: up to here dig_refine sums in LDS


# ---- the expected side ---------------------------------------------------------------------

def _set_bits(words, bits):
    """The bucket set's bits as a 0/1 array of 2**bits entries."""
    return np.unpackbits(np.asarray(words, np.uint64).view(np.uint8), bitorder="little")[:1 << bits].astype(np.int64)


def _model(ident, fp, bits, words, sub_bits):
    """(cells2 as (n_set << sub_bits, 2) uint64, member mask, each row's cell2 (members only valid), n_set)."""
    sb = _set_bits(words, bits)
    slot = np.cumsum(sb) - sb
    n_set = int(sb.sum())
    b = _buckets(ident, bits)
    member = sb[b] == 1
    sub = ((ident >> np.uint64(64 - bits - sub_bits)) & np.uint64((1 << sub_bits) - 1)).astype(np.int64)
    cell = (slot[b] << sub_bits) | sub
    cells2 = np.zeros((n_set << sub_bits, 2), np.uint64)
    np.add.at(cells2[:, 0], cell[member], np.uint64(1))
    np.add.at(cells2[:, 1], cell[member], fp[member])  # (wraps modulo 2^64)
    return cells2, member, cell, n_set


def _words_t(words):
    import torch
    return torch.from_numpy(np.asarray(words, np.uint64).view(np.int64).copy()).to(torch.device("cuda", 0))


def _refine(ctx, batch, bits, words, sub_bits, cap, alloc, n=None, spec=None, nbytes=None):
    """drp_digest_refine_device into `alloc` sentinel cells with cells_cap = cap: (cells as (alloc, 2)
    uint64, totals)."""
    import torch
    wire_t, cols = batch.device()
    cells = torch.full((max(alloc, 1), 2), SENTINEL, dtype=torch.int64, device=wire_t.device)
    tot = torch.full((3,), -1, dtype=torch.int64, device=wire_t.device)
    ctx.digest_refine_device(wire_t if nbytes is None else wire_t[:nbytes], cols, batch.n if n is None else n,
                             _filter(spec), bits, _words_t(words), sub_bits, cells, cap, tot)
    torch.cuda.synchronize()
    return cells.cpu().numpy().view(np.uint64)[:alloc], [int(v) for v in tot.cpu()]


def _check_refine(ctx, batch, bits, words, sub_bits, n=None, spec=None, nbytes=None, what=""):
    """The cells, the totals and the sentinel behind the cells against the model; returns (candidate
    rows, member mask, their cells, rows left out, n_set)."""
    idx, out = batch.candidates(n, spec, nbytes)
    want, member, cell, n_set = _model(batch.ident[idx], batch.fp[idx], bits, words, sub_bits)
    ncells = n_set << sub_bits
    got, tot = _refine(ctx, batch, bits, words, sub_bits, ncells + 3, ncells + 3, n, spec, nbytes)
    msg = f"bits {bits} sub_bits {sub_bits} {what} n {n} {spec}"
    assert tot == [int(member.sum()), len(out), n_set], msg
    np.testing.assert_array_equal(got[:ncells], want, err_msg=msg)
    assert np.all(got[ncells:] == np.uint64(SENTINEL)), msg
    return idx, member, cell, out, n_set


def _bucket_sets(bits):
    """Empty, full, a single bit at 0, 63, 64 and the last bucket (those that exist), a random half."""
    nb = 1 << bits
    sets = {"empty": [], "full": range(nb), "bit0": [0], "last": [nb - 1]}
    for b in (63, 64):
        if b < nb:
            sets[f"bit{b}"] = [b]
    sets["half"] = random.Random(bits).sample(range(nb), max(1, nb // 2))
    return {k: _set_words(v, bits) for k, v in sets.items()}


# ---- cells against the model -----------------------------------------------------------------

@pytest.mark.parametrize("sub_bits", [1, 4, 8])
@pytest.mark.parametrize("bits", [0, 1, 5, 6, 7, 16])
def test_cells_against_the_model(ctx, big, bits, sub_bits):
    """bits < 6: one word; 7: a rank that crosses a word; 16: the rank scan over 1024 words and every
    wave of its workgroup. The shared batch's value lengths put members and non-members of both hash
    paths into one wave. In LDS (few cells) and in global memory (bits 16)."""
    first = _digest(ctx, big, bits)[1]
    for name, words in _bucket_sets(bits).items():
        idx, member, _, out, n_set = _check_refine(ctx, big, bits, words, sub_bits, what=name)
        assert len(out) == first[1] == 0
        if name == "full":
            assert member.all() and n_set == 1 << bits
        if name == "empty":
            assert not member.any() and n_set == 0
        if name == "half" and bits:
            assert 0 < int(member.sum()) < len(idx)
            wide = big.ref["value_len"][idx] >= 256
            assert (wide & member).any() and (wide & ~member).any() and (~wide & member).any()


def test_lds_threshold(ctx, big):
    """The most cells summed in LDS and the fewest summed in global memory: 1024 (128 buckets of 8,
    64 buckets of 16) and 1040 (65 buckets of 16)."""
    held = sorted(set(_buckets(big.ident[big.candidates()[0]], 16).tolist()))  # buckets that hold rows
    for bits, buckets, sub_bits, ncells in [(7, range(128), 3, LDS_CELLS), (16, held[:64], 4, LDS_CELLS),
                                            (16, held[:65], 4, LDS_CELLS + 16)]:
        _, member, _, _, n_set = _check_refine(ctx, big, bits, _set_words(buckets, bits), sub_bits)
        assert n_set << sub_bits == ncells and int(member.sum()) >= 64


def test_roll_up(ctx, big):
    """The sub-cells of each slot sum to the device's own first-level cell of that bucket."""
    for bits, sub_bits in [(0, 8), (5, 4), (7, 1), (16, 2)]:
        first, _ = _digest(ctx, big, bits)
        for name in ["full", "half"]:
            words = _bucket_sets(bits)[name]
            set_buckets = np.flatnonzero(_set_bits(words, bits))
            ncells = len(set_buckets) << sub_bits
            got, tot = _refine(ctx, big, bits, words, sub_bits, ncells, ncells)
            rolled = got.reshape(len(set_buckets), 1 << sub_bits, 2).sum(axis=1, dtype=np.uint64)
            np.testing.assert_array_equal(rolled, first[set_buckets], err_msg=f"{bits} {sub_bits} {name}")
            assert tot[0] == int(first[set_buckets, 0].sum()) and tot[2] == len(set_buckets)


def test_capacity(ctx, big):
    """cells_cap one short of ncells, and 0: cells2 is entirely sentinel, totals complete. cells_cap =
    ncells: filled. In the LDS range of ncells and above it."""
    for bits, sub_bits in [(5, 4), (16, 4)]:
        words = _bucket_sets(bits)["half"]
        idx, _ = big.candidates()
        want, member, _, n_set = _model(big.ident[idx], big.fp[idx], bits, words, sub_bits)
        ncells = n_set << sub_bits
        assert (ncells <= LDS_CELLS) == (bits == 5)
        for cap in [ncells - 1, 0]:
            got, tot = _refine(ctx, big, bits, words, sub_bits, cap, ncells + 2)
            assert np.all(got == np.uint64(SENTINEL)), (bits, cap)
            assert tot == [int(member.sum()), 0, n_set]
        got, tot = _refine(ctx, big, bits, words, sub_bits, ncells, ncells + 2)
        np.testing.assert_array_equal(got[:ncells], want)
        assert np.all(got[ncells:] == np.uint64(SENTINEL)) and tot == [int(member.sum()), 0, n_set]


def test_no_rows(ctx, big):
    """n = 0: the cells of the set buckets are zeroed, the totals hold n_set."""
    words = _set_words([1, 5], 3)
    got, tot = _refine(ctx, big, 3, words, 2, 8, 10, n=0)
    assert not got[:8].any() and np.all(got[8:] == np.uint64(SENTINEL)) and tot == [0, 0, 2]


# ---- filters, n and truncated wires ------------------------------------------------------------

def test_filters_n_and_truncated_wires(ctx, big):
    """A change range, a key prefix, n below the row count, and nbytes cut inside a member's value (its
    key and subset still inside): that row is in no cell and is counted in totals[1], as are the rows
    behind the cut; totals[1] is the first level's whatever the set. The malformed row and the blob
    rows are in no cell."""
    ends = big.ends()
    r = big.ref
    k = next(i for i in range(3000, 4400) if big.ok[i] and r["flags"][i] & 2 and r["value_len"][i] >= 2
             and 3 <= int(r["change"][i]) <= 5
             and int(r["payload_off"][i]) + int(r["value_off"][i]) + int(r["value_len"][i]) == int(ends[i]))
    cut = int(ends[k]) - 1
    po = int(r["payload_off"][k])
    assert po + int(r["key_off"][k]) + int(r["key_len"][k]) <= cut  # (the value alone leaves the wire)
    assert not r["flags"][k] & 1 or po + int(r["subset_off"][k]) + int(r["subset_len"][k]) <= cut
    for bits, sub_bits in [(6, 4), (16, 8)]:
        half = set(np.flatnonzero(_set_bits(_bucket_sets(bits)["half"], bits)).tolist())
        words = _set_words(half | {int(_buckets(big.ident[k:k + 1], bits)[0])}, bits)  # (row k's bucket is set)
        for spec, n, nbytes in [({"change_range": (3, 5)}, None, None), ({"key_prefix": b"k1"}, None, None),
                                (None, 3000, None), (None, None, cut), ({"change_range": (2, 8)}, 4500, cut)]:
            idx, member, _, out, _ = _check_refine(ctx, big, bits, words, sub_bits, n, spec, nbytes)
            assert 0 < int(member.sum()) < len(idx)
            assert 2500 not in idx and not np.any(idx % 50 == 49)  # the malformed row, the blobs
            assert len(out) == _digest(ctx, big, bits, n, spec, nbytes)[1][1]
            if nbytes is not None:
                assert k in out and k not in idx and len(out) > 1
            else:
                assert len(out) == 0
        # the first level's count of rows left out, whatever the set
        for name in ["empty", "full"]:
            *_, out, _ = _check_refine(ctx, big, bits, _bucket_sets(bits)[name], sub_bits, nbytes=cut)
            assert k in out


# ---- cell diff ---------------------------------------------------------------------------------

def _diff_cells(ctx, a, b, ncells):
    """drp_digest_diff_cells_device of two (ncells, 2) uint64 arrays: (set words as uint64, n_diff)."""
    import torch
    dev = torch.device("cuda", 0)
    pad = lambda x: np.ascontiguousarray(x if ncells else np.zeros((1, 2), np.uint64))
    up = lambda x: torch.from_numpy(pad(x).view(np.int64).copy()).to(dev)
    nw = max(1, (ncells + 63) // 64)
    cset = torch.full((nw + 1,), -1, dtype=torch.int64, device=dev)
    nd = torch.full((1,), -1, dtype=torch.int64, device=dev)
    ctx.digest_diff_cells_device(up(a), up(b), ncells, cset, nd)
    torch.cuda.synchronize()
    w = cset.cpu().numpy().view(np.uint64)
    assert w[nw] == np.uint64(M64)  # (nothing behind the set's words is written)
    return w[:nw], int(nd.cpu()[0])


def _cell_words(cells, ncells):
    """The cell set of `cells` (ALL: every one of the ncells) as uint64 words."""
    w = np.zeros(max(1, (ncells + 63) // 64), np.uint64)
    if cells is ALL:
        bits = np.zeros(len(w) * 64, np.uint8)
        bits[:ncells] = 1
        return np.packbits(bits, bitorder="little").view(np.uint64)
    for c in cells:
        w[c >> 6] |= np.uint64(1 << (c & 63))
    return w


ALL = "all"


@pytest.mark.parametrize("ncells", [0, 1, 20, 64, 65, 260, 65536 << 4])
def test_cell_diff(ctx, ncells):
    """Equal cells: the empty set. Differences in the first cell, the last cell and either side of
    every word boundary there is among the first 260 cells, in count only and in sum only: exactly
    those bits, the high bits of the last word 0, n_diff exact. Every cell altered: every bit."""
    rng = np.random.default_rng(ncells)
    a = rng.integers(0, 1 << 63, size=(ncells, 2), dtype=np.uint64)
    cset, nd = _diff_cells(ctx, a, a, ncells)
    assert nd == 0 and not cset.any()
    pick = sorted({c for c in [0, 63, 64, 127, 128, 255, 256, ncells - 64, ncells - 65, ncells - 1] if 0 <= c < ncells})
    b = a.copy()
    for j, c in enumerate(pick):
        b[c, j % 2] ^= np.uint64(1 << 63)
    cset, nd = _diff_cells(ctx, a, b, ncells)
    assert nd == len(pick)
    np.testing.assert_array_equal(cset, _cell_words(pick, ncells))
    if ncells:
        b = a.copy()
        b[:, 1] += np.uint64(1)
        cset, nd = _diff_cells(ctx, b, a, ncells)
        assert nd == ncells
        bits = np.unpackbits(cset.view(np.uint8), bitorder="little")
        assert bits[:ncells].all() and not bits[ncells:].any()


# ---- refined select ----------------------------------------------------------------------------

def _select_refined(ctx, batch, bits, words, sub_bits, cset, n=None, spec=None, nbytes=None):
    """drp_select_refined_device into poisoned outputs: (rows, sel_idx)."""
    import torch
    wire_t, cols = batch.device()
    n = batch.n if n is None else n
    dev = wire_t.device
    rows = {k: torch.full((max(n, 1),), 0x55, dtype=(torch.int32 if k.endswith("_len") else
                                                     torch.uint8 if k == "flags" else torch.int64), device=dev)
            for k in SRC_KEYS}
    idx_t = torch.full((max(n, 1),), -1, dtype=torch.int64, device=dev)
    nsel_t = torch.full((1,), -1, dtype=torch.int64, device=dev)
    ctx.select_refined_device(wire_t if nbytes is None else wire_t[:nbytes], cols, n, _filter(spec), bits, _words_t(words),
                              sub_bits, _words_t(cset), rows, idx_t, nsel_t)
    torch.cuda.synchronize()
    nsel = int(nsel_t.cpu()[0])
    assert np.all(idx_t.cpu().numpy()[nsel:] == -1)
    return {k: v.cpu().numpy()[:nsel] for k, v in rows.items()}, idx_t.cpu().numpy()[:nsel]


def _check_select(ctx, batch, bits, words, sub_bits, keep_cells, n=None, spec=None, nbytes=None):
    """The rows kept are the model's rows of the cells in keep_cells, in row order; returns them."""
    idx, _ = batch.candidates(n, spec, nbytes)
    _, member, cell, n_set = _model(batch.ident[idx], batch.fp[idx], bits, words, sub_bits)
    ncells = n_set << sub_bits
    want = idx[member] if keep_cells is ALL else idx[member & np.isin(cell, list(keep_cells))]
    got, sel = _select_refined(ctx, batch, bits, words, sub_bits, _cell_words(keep_cells, ncells), n, spec, nbytes)
    _check_rows(batch, got, sel, want, (bits, sub_bits, n, spec))
    assert np.all(np.diff(sel) > 0)  # stable: the source rows' order
    return want, ncells


def test_refined_select(ctx, big):
    """Rows and sel_idx equal the model's: exactly the rows the refine counted in the set cells, in
    row order. Every cell set: the bucket select's rows. An empty cell_set and an empty bucket_set
    select nothing. With a filter, rows [0, n) only, and a truncated wire."""
    cut = int(big.ends()[4000]) - 1
    for bits, sub_bits in [(0, 8), (5, 1), (7, 4), (16, 8)]:
        words = _bucket_sets(bits)["half"]
        idx, _ = big.candidates()
        cells2, member, cell, n_set = _model(big.ident[idx], big.fp[idx], bits, words, sub_bits)
        ncells = n_set << sub_bits
        live = np.flatnonzero(cells2[:, 0])
        keep = sorted(random.Random(bits).sample(live.tolist(), max(1, len(live) // 2)))
        for spec, n, nbytes in [(None, None, None), ({"change_range": (2, 6)}, None, None), (None, 1025, None),
                                ({"key_prefix": b"k1"}, 4500, cut)]:
            want, _ = _check_select(ctx, big, bits, words, sub_bits, keep, n, spec, nbytes)
            assert len(want) > 0
        want, _ = _check_select(ctx, big, bits, words, sub_bits, keep)
        assert len(want) == int(cells2[keep, 0].sum()) < int(member.sum())  # the rows counted in those cells
        want, _ = _check_select(ctx, big, bits, words, sub_bits, ALL)
        np.testing.assert_array_equal(want, idx[member])
        want, _ = _check_select(ctx, big, bits, words, sub_bits, [])
        assert len(want) == 0
        want, ncells0 = _check_select(ctx, big, bits, _bucket_sets(bits)["empty"], sub_bits, [])
        assert len(want) == 0 and ncells0 == 0
    got, sel = _select_refined(ctx, big, 4, _set_words([3], 4), 2, _cell_words([1], 4), n=0)
    assert len(sel) == 0


def test_hash_mask_does_not_reach_the_refined_calls(ctx, big):
    """drp_set_latest_hash_mask(0) changes neither the cells nor the refined select."""
    words = _bucket_sets(6)["half"]
    try:
        for mask in [0, M64]:
            ctx.set_latest_hash_mask(mask)
            _, member, cell, _, n_set = _check_refine(ctx, big, 6, words, 4)
            keep = sorted(set(cell[member].tolist()))[::3]
            _check_select(ctx, big, 6, words, 4, keep)
    finally:
        ctx.set_latest_hash_mask(M64)


def test_invalid_arguments(ctx, big):
    import torch
    from _gpu import drp_amd
    wire_t, cols = big.device()
    z = torch.zeros(1 << 12, dtype=torch.int64, device=wire_t.device)
    rows = {k: torch.zeros(big.n, dtype=(torch.int32 if k.endswith("_len") else torch.uint8 if k == "flags" else
                                         torch.int64), device=wire_t.device) for k in SRC_KEYS}
    for bits, bset, sub_bits, cells2, tot in [(17, z, 1, z, z), (4, None, 1, z, z), (4, z, 0, z, z), (4, z, 9, z, z),
                                              (4, z, 1, None, z), (4, z, 1, z, None)]:
        with pytest.raises(drp_amd.DrpError) as e:
            ctx.digest_refine_device(wire_t, cols, big.n, None, bits, bset, sub_bits, cells2, 16, tot)
        assert e.value.rc == drp_amd.DRP_E_INVAL
    for a, b, ncells, cset, nd in [(z, z, (65536 << 8) + 1, z, z), (z, z, 4, None, z), (z, z, 4, z, None)]:
        with pytest.raises(drp_amd.DrpError) as e:
            ctx.digest_diff_cells_device(a, b, ncells, cset, nd)
        assert e.value.rc == drp_amd.DRP_E_INVAL
    for bits, bset, sub_bits, cset, out, nsel in [(17, z, 1, z, rows, z), (4, None, 1, z, rows, z), (4, z, 0, z, rows, z),
                                                  (4, z, 9, z, rows, z), (4, z, 1, None, rows, z), (4, z, 1, z, None, z),
                                                  (4, z, 1, z, rows, None)]:
        with pytest.raises(drp_amd.DrpError) as e:
            ctx.select_refined_device(wire_t, cols, big.n, None, bits, bset, sub_bits, cset, out, None, nsel)
        assert e.value.rc == drp_amd.DRP_E_INVAL


# ---- several chunks per workgroup --------------------------------------------------------------

def test_several_chunks_per_workgroup(ctx):
    """From 2 * 128 * 1024 rows on a dig_refine workgroup takes more than one chunk of 1024 rows, as
    dig_cells does (DIG_CHUNKS, DIG_GRID_MIN of drp_kernels.h). 270,001 Changes of the C2 shape
    (10-digit keys, 64 value bytes, no subset), the expected side as test_gpu_digest's. In LDS and in
    global memory; the refined select over the same rows."""
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
    for bits, sub_bits in [(5, 4), (12, 4)]:
        words = _bucket_sets(bits)["half"]
        want, member, cell, n_set = _model(ident, h, bits, words, sub_bits)
        ncells = n_set << sub_bits
        assert (ncells <= LDS_CELLS) == (bits == 5)
        cells = torch.full((ncells + 1, 2), SENTINEL, dtype=torch.int64, device=dev)
        tot = torch.full((3,), -1, dtype=torch.int64, device=dev)
        ctx.digest_refine_device(wire_t, cols, n, None, bits, _words_t(words), sub_bits, cells, ncells, tot)
        torch.cuda.synchronize()
        got = cells.cpu().numpy().view(np.uint64)
        np.testing.assert_array_equal(got[:ncells], want)
        assert np.all(got[ncells:] == np.uint64(SENTINEL))
        assert [int(v) for v in tot.cpu()] == [int(member.sum()), 0, n_set]
        keep = np.flatnonzero(want[:, 0])[::2]
        idx_t = torch.full((n,), -1, dtype=torch.int64, device=dev)
        nsel_t = torch.full((1,), -1, dtype=torch.int64, device=dev)
        rows = {k: torch.zeros(n, dtype=(torch.int32 if k.endswith("_len") else torch.uint8 if k == "flags" else
                                         torch.int64), device=dev) for k in SRC_KEYS}
        ctx.select_refined_device(wire_t, cols, n, None, bits, _words_t(words), sub_bits,
                                  _words_t(_cell_words(keep.tolist(), ncells)), rows, idx_t, nsel_t)
        torch.cuda.synchronize()
        sel = idx_t.cpu().numpy()[:int(nsel_t.cpu()[0])]
        np.testing.assert_array_equal(sel, np.flatnonzero(member & np.isin(cell, keep)))


# ---- end to end --------------------------------------------------------------------------------

def _model_cells2(rows, bits, words, sub_bits):
    ident, fp = _hashes(rows)
    return _model(ident, fp, bits, words, sub_bits)


def test_end_to_end(ctx):
    """The two stores of test_gpu_digest's end to end (about 2000 identities that differ in 5) at bits
    = 4, where a bucket holds about 125 keys and the first level alone sends hundreds of rows, refined
    by sub_bits = 8. Each side: digest, diff, digest_refined, reconcile_refined against the other's
    cells2. The bytes decode to exactly the model's rows of the differing cells, in store order: at
    least that side's truly differing identities, strictly fewer rows than Store.reconcile sends.
    After each side merges the other's bytes both first-level digests are equal, and equal to the
    digest of the latest per key over the union. A refined reconcile of equal stores sends nothing."""
    rng = random.Random(31)
    bits, sub_bits = 4, 8
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
    # the model: first-level diff, second-level cells, their diff, the rows of the differing cells
    ca, cb = _cells_of(ma.rows, bits), _cells_of(mb.rows, bits)
    differ = np.flatnonzero((ca != cb).any(axis=1))
    assert 3 <= len(differ) <= 5
    words = _set_words(differ.tolist(), bits)
    m2a, mem_a, cell_a, n_set = _model_cells2(ma.rows, bits, words, sub_bits)
    m2b, mem_b, cell_b, _ = _model_cells2(mb.rows, bits, words, sub_bits)
    differ2 = np.flatnonzero((m2a != m2b).any(axis=1))
    want_a = [c for c, m, ce in zip(ma.rows, mem_a, cell_a) if m and ce in set(differ2.tolist())]
    want_b = [c for c, m, ce in zip(mb.rows, mem_b, cell_b) if m and ce in set(differ2.tolist())]
    first_a, first_b = int(mem_a.sum()), int(mem_b.sum())  # what Store.reconcile sends at these bits
    assert 4 <= len(want_a) < first_a and 3 <= len(want_b) < first_b and first_a > 300  # (the input shows it)
    # the device
    da, db = A.digest(bits), B.digest(bits)
    bset, nd = _diff(ctx, da.cpu().numpy().view(np.uint64), db.cpu().numpy().view(np.uint64), bits)
    np.testing.assert_array_equal(bset, words)
    assert nd == len(differ)
    c2a, ns_a = A.digest_refined(bits, bset, sub_bits)  # (a numpy array as well as a tensor)
    c2b, ns_b = B.digest_refined(bits, _words_t(bset), sub_bits)
    assert ns_a == ns_b == n_set and tuple(c2a.shape) == (n_set << sub_bits, 2)
    np.testing.assert_array_equal(c2a.cpu().numpy().view(np.uint64), m2a)
    np.testing.assert_array_equal(c2b.cpu().numpy().view(np.uint64), m2b)
    wire_a, cells_a = A.reconcile_refined(c2b, bits, bset, sub_bits)
    wire_b, cells_b = B.reconcile_refined(c2a.cpu().numpy(), bits, _words_t(bset), sub_bits)
    np.testing.assert_array_equal(cells_a, differ2)
    np.testing.assert_array_equal(cells_b, differ2)
    for wire, want in [(wire_a, want_a), (wire_b, want_b)]:
        ref = O.decode_batch(wire)
        assert ref["err_code"] == 0 and ref["consumed"] == len(wire)
        assert [_change(wire, ref, i) for i in range(ref["nframes"])] == want
    for store, peer, want, first in [(A, db, want_a, first_a), (B, da, want_b, first_b)]:
        sent = O.decode_batch(store.reconcile(peer, bits)[0])["nframes"]
        assert sent == first > len(want)
    _, cnt = _merge(ctx, B, mb, wire_a)
    assert (cnt["inserted"], cnt["replaced"], cnt["stale"], cnt["unchanged"]) == (2, 2, 0, len(want_a) - 4)
    _, cnt = _merge(ctx, A, ma, wire_b)
    assert (cnt["inserted"], cnt["replaced"], cnt["stale"], cnt["unchanged"]) == (1, 0, 2, len(want_b) - 3)
    union = _cells_of(_winners(_wire(rows_a + rows_b))[1], bits)
    np.testing.assert_array_equal(A.digest(bits).cpu().numpy().view(np.uint64), union)
    np.testing.assert_array_equal(B.digest(bits).cpu().numpy().view(np.uint64), union)
    # equal stores: the empty bucket set sends nothing, and so does a refine of every bucket
    bset, nd = _diff(ctx, A.digest(bits).cpu().numpy().view(np.uint64), B.digest(bits).cpu().numpy().view(np.uint64), bits)
    assert nd == 0
    for s in [bset, _set_words(range(1 << bits), bits)]:
        wire, cells = A.reconcile_refined(B.digest_refined(bits, s, sub_bits)[0], bits, s, sub_bits)
        assert wire == b"" and len(cells) == 0
