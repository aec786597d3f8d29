"""GPU parity for the key-ordered listing (drp_order_keys_device, Store.list_keys): the encoder rows of
every segment of a fan-out's output in ascending (key bytes, subset absent first, subset bytes, input
position), restricted to a key range, cut to a limit, the outputs end to end. Every comparison is
exact. There is no reference counterpart; the expected side is Python's sorted() over that tuple
(_model below), then the bounds and the cut; Store.list_keys' bytes are decoded with the oracle and
compared row by row."""
import collections

import numpy as np
import pytest

import _oracle as O
import _streams as S
from _relay import SRC_KEYS as SRC, U64MAX, Change, change_at, down as _down, dtype as _dtype, up as _up

pytestmark = pytest.mark.gpu

GUARD = 0x5A
TILE, SCAN = 4096, 1024  # the sort workgroup's pairs and the counts of one first-level scan block
MAXB = 4096


@pytest.fixture(scope="module")
def ctx():
    from _gpu import drp_amd
    assert (drp_amd.ORDER_TILE, drp_amd.ORDER_SCAN, drp_amd.KEYORDER_MAX_BYTES) == (TILE, SCAN, MAXB)
    c = drp_amd.Ctx(0)
    yield c
    c.close()


# ---- inputs, the call, the expected side ---------------------------------------------------------

class Rows:
    """Encoder rows over a heap built from (key, subset or None) pairs: the strings lie in the heap in
    row order, each after `gap(i)` bytes of 0xEE filler (so a string's neighbours are never zero and
    every alignment occurs), the heap ends with the last string's last byte. Every other column is a
    different function of the row index. cap: the arrays' entries (>= the rows)."""

    def __init__(self, pairs, cap=None, gap=lambda i: (i * 5 + 1) % 4, change=None, tail=b""):
        self.keys = [bytes(k) for k, _ in pairs]
        self.subs = [None if s is None else bytes(s) for _, s in pairs]
        n = len(pairs)
        cap = n if cap is None else cap
        i = np.arange(cap, dtype=np.uint64)
        c = {"key_off": np.zeros(cap, np.uint64), "key_len": np.zeros(cap, np.uint64),
             "subset_off": (i << np.uint64(33)) + np.uint64(3), "subset_len": i % np.uint64(97),
             "value_off": i * np.uint64(13) + np.uint64(5), "value_len": (i * np.uint64(5)) % np.uint64(1001),
             "change": i * np.uint64(3) % np.uint64(11), "from": i ^ np.uint64(0x5555), "to": i * np.uint64(2) + np.uint64(9),
             "flags": (i % np.uint64(2)) * np.uint64(2)}  # (DRP_F_VALUE on every other row: not the order's business)
        if change is not None:
            c["change"][:n] = np.asarray(change, np.uint64)
        heap = bytearray()
        for r, (k, s) in enumerate(zip(self.keys, self.subs)):
            # (the subset first: the key of the last row is the heap's last string)
            if s is not None:
                heap += b"\xEE" * gap(2 * r)
                c["subset_off"][r], c["subset_len"][r] = len(heap), len(s)
                c["flags"][r] |= np.uint64(1)
                heap += s
            heap += b"\xEE" * gap(2 * r + 1)
            c["key_off"][r], c["key_len"][r] = len(heap), len(k)
            heap += k
        heap += tail
        self.heap = np.frombuffer(bytes(heap), np.uint8).copy()
        self.cols = {k: v.astype(_dtype(k)) for k, v in c.items()}
        self.n, self.cap = n, cap
        self.bad = set()  # rows the test has put out of the heap or over the cap (the model leaves them out)


def _guards(cap, K):
    full = lambda n, dt: np.full(n * np.dtype(dt).itemsize, GUARD, np.uint8).view(dt)
    return {k: full(max(cap, 1), _dtype(k)) for k in SRC}, full(max(cap, 1), np.uint64), full(K + 1, np.uint64)


def _pages(pages):
    from _gpu import drp_amd
    if pages is None:
        return None
    return [None if g is None else drp_amd.make_key_page(**g) for g in pages]


def _call(ctx, R, base, pages=None, keep_ties=False, sel=True, c=None):
    """One drp_order_keys_device; every output array starts as a guard pattern. Returns (out_rows,
    out_sel_idx, out_base, totals) as numpy arrays, whole."""
    c = c or ctx
    K = len(base) - 1
    g_rows, g_sel, g_base = _guards(R.cap, K)
    d_rows = {k: _up(v if len(v) else np.zeros(1, v.dtype)) for k, v in R.cols.items()}
    d_out = {k: _up(v) for k, v in g_rows.items()}
    d_sel = _up(np.arange(max(R.cap, 1), dtype=np.uint64)) if sel else None
    d_osel = _up(g_sel) if sel else None
    d_base, d_obase = _up(np.asarray(base, np.uint64)), _up(g_base)
    d_tot = _up(np.full(2, 77, np.uint64))
    d_heap = _up(R.heap) if len(R.heap) else None  # (sized exactly)
    c.order_keys_device(d_heap, d_rows, d_base, K, R.cap, d_out, d_obase, pages=_pages(pages), keep_ties=keep_ties,
                        sel_idx_t=d_sel, out_sel_idx_t=d_osel, totals_t=d_tot)
    return {k: _down(v) for k, v in d_out.items()}, _down(d_osel) if sel else None, _down(d_obase), _down(d_tot)


def _model(R, base, pages=None, keep_ties=False):
    """(the source row of every output row, out_base, totals): per segment the sorted() of the issue,
    the bounds on the key, the limit, the tie rule."""
    key, sub = R.keys, R.subs
    K = len(base) - 1
    perm, ob, took = [], [0], 0
    for f in range(K):
        rows = [i for i in range(int(base[f]), int(base[f + 1])) if i not in R.bad]
        took += len(rows)
        order = sorted(rows, key=lambda i: (key[i], sub[i] is not None, sub[i] if sub[i] is not None else b"", i))
        g = (pages[f] if pages is not None else None) or {}
        if g.get("from_") is not None:
            order = [i for i in order if key[i] >= g["from_"]]
        if g.get("after") is not None:
            order = [i for i in order if key[i] > g["after"]]
        if g.get("until") is not None:
            order = [i for i in order if key[i] < g["until"]]
        lim = g.get("limit")
        kept = len(order) if lim is None else min(len(order), lim)
        if keep_ties and 0 < kept < len(order):
            while kept < len(order) and key[order[kept]] == key[order[kept - 1]]:
                kept += 1
        perm += order[:kept]
        ob.append(ob[-1] + kept)
    n_in = int(base[-1]) - int(base[0])
    return np.array(perm, np.int64), np.array(ob, np.uint64), np.array([took, n_in - took], np.uint64)


def _check(ctx, R, base=None, pages=None, keep_ties=False, c=None):
    """One call against the model: out_base entry by entry, totals, every column of every kept row,
    sel_idx, and the guard pattern at and beyond out_base[nseg]. Returns (perm, out_base)."""
    base = [0, R.n] if base is None else base
    out, osel, obase, tot = _call(ctx, R, base, pages, keep_ties, c=c)
    perm, want_base, want_tot = _model(R, base, pages, keep_ties)
    np.testing.assert_array_equal(obase, want_base)
    np.testing.assert_array_equal(tot, want_tot)
    total = len(perm)
    np.testing.assert_array_equal(osel[:total], perm.astype(np.uint64))
    g_rows, g_sel, _ = _guards(R.cap, len(base) - 1)
    np.testing.assert_array_equal(osel[total:], g_sel[total:])
    for k in SRC:
        np.testing.assert_array_equal(out[k][:total], R.cols[k][perm], err_msg=k)
        np.testing.assert_array_equal(out[k][total:], g_rows[k][total:], err_msg=k + " (guard)")
    return perm, want_base


ALPHA = [0x00, 0x01, 0x61, 0x62, 0x7F, 0x80, 0xFF]  # few byte values: shared prefixes and equal keys are common


def _random_pairs(n, seed, max_len=20):
    rng = np.random.default_rng(seed)
    subs = [None, b"", b"a", b"ab", b"b"]
    out = []
    for ln, si in zip(rng.integers(0, max_len + 1, size=n), rng.integers(0, len(subs), size=n)):
        out.append((bytes(rng.choice(ALPHA, size=int(ln)).astype(np.uint8)), subs[int(si)]))
    return out


# ---- row counts and tile edges ---------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_row_counts(ctx, n):
    """One segment of n rows with random keys of 0 to 20 bytes: 0, 1, the wave, the sort workgroup's
    tile and two tiles, one below, at and one above; the arrays hold five entries more than the rows."""
    _check(ctx, Rows(_random_pairs(n, n), cap=n + 5))


def test_scan_past_one_block(ctx):
    """A pass's count table holds 256 * ceil(n / TILE) counts, scanned in first-level blocks of SCAN:
    it passes one block from five workgroups on, n = 4 * TILE + 1 the smallest."""
    n = 4 * TILE + 1
    assert 256 * ((n + TILE - 1) // TILE) > SCAN >= 256 * ((n - 1) // TILE)
    R = Rows(_random_pairs(n, 7, max_len=9))
    _check(ctx, R)
    _check(ctx, R, base=[0, 5, TILE + 3, TILE + 3, 3 * TILE, n])


# ---- words, padding, unsigned bytes, the heap's end ----------------------------------------------------

def test_word_edges_and_alignments(ctx):
    """Key lengths 0, 1, 7, 8, 9, 15, 16, 17 and 24 in one segment, each at every alignment 0 to 7 within
    the heap (the filler before a key is chosen so), several keys per length that differ only in their
    last byte or are equal."""
    rng = np.random.default_rng(11)
    pairs = []
    for ln in [0, 1, 7, 8, 9, 15, 16, 17, 24]:
        stem = bytes(rng.integers(0, 256, size=ln, dtype=np.uint8))
        for a in range(8):
            pairs.append((stem[:-1] + bytes([(stem[-1] + a // 2) % 256]) if ln else b"", None))
    order = rng.permutation(len(pairs))
    pairs = [pairs[i] for i in order]
    # row r's key starts at alignment r % 8: the columns from Rows, the heap laid out here
    R = Rows(pairs, gap=lambda j: 0)
    offs, at = [], 0
    for r, (k, _) in enumerate(pairs):
        at += (r - at) % 8
        offs.append(at)
        at += len(k)
    heap = bytearray(b"\xEE" * at)
    for o, (k, _) in zip(offs, pairs):
        heap[o:o + len(k)] = k
    R.heap = np.frombuffer(bytes(heap), np.uint8).copy()
    R.cols["key_off"] = np.array(offs, np.uint64)
    assert {o % 8 for o in offs} == set(range(8))
    _check(ctx, R)


PAD = [b"", b"\0", b"\0\0", b"ab", b"ab\0", b"ab\0\0", b"ab\x01"]


def test_padding_hazard(ctx):
    """A zero-padded word cannot tell "ab" from "ab\\0": the length must. The same with the split at
    byte 8, a word boundary, and at byte 16; every string twice (a tie) and in reverse order."""
    e8, e16 = b"12345678", b"12345678abcdefgh"
    keys = PAD + [e8, e8 + b"\0", e8 + b"\0\0", e8 + b"\x01", e8[:7], e16, e16 + b"\0", e16 + b"\x01", e16[:15]]
    pairs = [(k, None) for k in (keys + keys)[::-1]]
    perm, _ = _check(ctx, Rows(pairs))
    got = [pairs[i][0] for i in perm]
    assert [k for k in got if k in PAD][::2] == PAD and got == sorted(got)
    i8 = got.index(e8)
    assert got[i8:i8 + 8:2] == [e8, e8 + b"\0", e8 + b"\0\0", e8 + b"\x01"]


def test_unsigned_bytes(ctx):
    """0x00, 0x7F, 0x80 and 0xFF in the first position of a word, in its last position, and in the last
    byte of a key (of 1, 8, 9, 12 and 16 bytes): a signed compare of bytes or of words would put 0x80
    and 0xFF first."""
    vals = [0x00, 0x7F, 0x80, 0xFF]
    stem = b"ABCDEFGHIJKLMNOP"
    keys = []
    for pos, ln in [(0, 1), (0, 8), (7, 8), (8, 9), (8, 16), (15, 16), (11, 12), (0, 16), (7, 16)]:
        for v in vals:
            k = bytearray(stem[:ln])
            k[pos] = v
            keys.append(bytes(k))
    rng = np.random.default_rng(12)
    pairs = [(keys[i], None) for i in rng.permutation(len(keys))]
    perm, _ = _check(ctx, Rows(pairs))
    got = [pairs[i][0] for i in perm]
    assert got == sorted(keys)
    one = [k for k in got if len(k) == 1]
    assert one == [b"\x00", b"\x7f", b"\x80", b"\xff"]


@pytest.mark.parametrize("last_len", [1, 3, 5, 8])
def test_heap_end(ctx, last_len):
    """The heap tensor is sized exactly and the greatest key ends at its last byte, its last word
    partial (or, at 8, whole and flush with the end): the order is still right, and a key one byte
    longer than the heap allows is left out instead of read."""
    pairs = _random_pairs(200, 40 + last_len, max_len=12) + [(b"\xFF" * (16 + last_len), None)]
    R = Rows(pairs)
    assert int(R.cols["key_off"][-1]) + 16 + last_len == len(R.heap)
    perm, _ = _check(ctx, R)
    assert perm[-1] == len(pairs) - 1
    R.cols["key_len"][-1] += 1
    R.bad.add(len(pairs) - 1)
    _check(ctx, R)


# ---- skipped words and digits ------------------------------------------------------------------------

def _skip_cases():
    rng = np.random.default_rng(13)
    prefix = b"tenant-0001/users/x"  # 19 bytes: two whole words and three bytes of the third
    assert len(prefix) == 19
    differ = [(prefix + bytes([int(b)]) + b"tail", None) for b in rng.integers(0, 256, size=600)]
    equal = [(prefix + b"same", None if i % 3 else b"s") for i in range(600)]
    shorter = differ[:200] + [(prefix[:16], None), (prefix[:9], None), (prefix[:8], None)] + differ[200:400]
    other_first = [(b"zz", None)] + differ[:300]
    return {"differ_in_byte_19": differ, "all_equal": equal, "all_equal_no_subset": [(b"k", None)] * 300,
            "prefix_and_shorter": shorter, "first_row_differs": other_first}


@pytest.mark.parametrize("case", ["differ_in_byte_19", "all_equal", "all_equal_no_subset", "prefix_and_shorter",
                                  "first_row_differs"])
def test_skipped_words(ctx, case, monkeypatch):
    """All keys share a 19-byte prefix and differ in byte 19; all keys equal (the subset, then the
    position decide); all rows equal (only the position decides); the prefix shared by all but three
    keys that end inside it, at and one past a word boundary; by all but the first row. The leading key
    words every row shares are never launched and the digits in which no two rows differ are switched
    off on the device; with DRP_ORDER_SKIP=0 (read when a ctx opens) every digit
    of every word runs: the output is identical."""
    from _gpu import drp_amd
    R = Rows(_skip_cases()[case])
    base = [0, 250, 250, R.n]
    a = _call(ctx, R, base)
    _check(ctx, R, base)
    monkeypatch.setenv("DRP_ORDER_SKIP", "0")
    c = drp_amd.Ctx(0)
    try:
        b = _call(ctx, R, base, c=c)
        _check(ctx, R, base, c=c)
    finally:
        c.close()
    for k in SRC:
        np.testing.assert_array_equal(a[0][k], b[0][k], err_msg=k)
    for x, y in zip(a[1:], b[1:]):
        np.testing.assert_array_equal(x, y)


# ---- long keys, rows left out ----------------------------------------------------------------------------

def test_one_long_key(ctx):
    """One key of 4096 bytes among keys of 4 bytes takes part (512 words for one row); one of 4097 is
    left out: totals == [n - 1, 1] and the others are sorted. The same for a subset of 4097 bytes."""
    short = [(bytes([97 + i % 5, 97 + i % 3, 97 + i % 7, 97 + i % 2]), None) for i in range(70)]
    long_key = b"cab" + b"\0" * (MAXB - 4) + b"\x01"
    R = Rows(short[:30] + [(long_key, None)] + short[30:])
    perm, _ = _check(ctx, R)
    assert len(perm) == 71 and 30 in perm
    R = Rows(short[:30] + [(long_key + b"z", None)] + short[30:])
    R.bad.add(30)
    out, _, obase, tot = _call(ctx, R, [0, R.n])
    assert list(tot) == [70, 1] and list(obase) == [0, 70]
    _check(ctx, R)
    R = Rows(short[:30] + [(b"cab", b"s" * (MAXB + 1))] + short[30:])
    R.bad.add(30)
    _check(ctx, R, base=[0, 10, R.n])
    R = Rows(short[:30] + [(b"cab", b"s" * MAXB)] + short[30:])
    _check(ctx, R, base=[0, 10, R.n])


def test_out_of_heap(ctx):
    """A key range that leaves the heap (by one byte; by an offset near 2^64), a subset
    range that does while DRP_F_SUBSET is set: the row is left out, counted, and never read. The same
    subset range without the flag: the row takes part."""
    pairs = _random_pairs(300, 17, max_len=10)
    R = Rows(pairs, tail=b"")
    hb = len(R.heap)
    R.cols["key_off"][5] = hb - 2
    R.cols["key_len"][5] = 3
    R.cols["key_off"][7] = U64MAX - 1
    R.cols["key_len"][7] = 4
    R.cols["key_off"][0] = hb  # (the first row, the one the shared prefix is counted against)
    R.cols["key_len"][0] = 1
    R.bad |= {0, 5, 7}
    with_sub = [i for i in range(20, 300) if R.subs[i] is not None][:2]
    without = [i for i in range(20, 300) if R.subs[i] is None][:2]
    for i in with_sub:
        R.cols["subset_off"][i] = hb - 1
        R.cols["subset_len"][i] = 2
        R.bad.add(i)
    for i in without:  # (Rows leaves subset_off of such rows far outside the heap already)
        assert int(R.cols["subset_off"][i]) > hb and not R.cols["flags"][i] & 1
    _, obase, tot = _call(ctx, R, [0, 100, 300])[1:]
    assert list(tot) == [295, 5] and int(obase[-1]) == 295
    perm, _ = _check(ctx, R, base=[0, 100, 300])
    assert set(without) <= set(perm.tolist()) and not R.bad & set(perm.tolist())
    # a row left out is not counted against a limit, and bounds see only the rows that took part
    _check(ctx, R, base=[0, 100, 300], pages=[{"limit": 97}, {"from_": b"\x01", "limit": 150}], keep_ties=True)
    # no heap at all: only empty keys take part
    E = Rows([(b"", None), (b"", b""), (b"", None)], gap=lambda j: 0)
    assert len(E.heap) == 0
    _check(ctx, E)
    E.cols["key_len"][1] = 1
    E.bad.add(1)
    _check(ctx, E)


# ---- the subset tie-break, stability ------------------------------------------------------------------------

def test_subset_tie_break(ctx):
    """One key under the subsets absent, present and empty, "a", "ab", "b" (and a second key around
    it): absent first, then the subsets in byte order, whatever the input order."""
    subs = [b"b", None, b"ab", b"", b"a"]
    pairs = [(b"k", s) for s in subs] + [(b"j", b"zz"), (b"l", None), (b"k\0", None)]
    perm, _ = _check(ctx, Rows(pairs))
    assert [pairs[i] for i in perm] == [(b"j", b"zz"), (b"k", None), (b"k", b""), (b"k", b"a"), (b"k", b"ab"),
                                        (b"k", b"b"), (b"k\0", None), (b"l", None)]
    # subsets that differ past a word, and by their length only
    s8 = b"subset88"
    pairs = [(b"k", s) for s in [s8 + b"\0", s8, s8 + b"\x01", s8[:7], s8 + b"\0\0", None]]
    perm, _ = _check(ctx, Rows(pairs))
    assert [pairs[i][1] for i in perm] == [None, s8[:7], s8, s8 + b"\0", s8 + b"\0\0", s8 + b"\x01"]


def test_stable(ctx):
    """Several rows of one identity with different `change` (5,000 rows over 7 identities, sel_idx =
    arange): within an identity out_sel_idx increases, whatever the changes say."""
    n = 5000
    ids = [(b"key-%d" % (i % 4), b"s" if i % 7 == 0 else None) for i in range(n)]
    R = Rows(ids, change=np.random.default_rng(5).integers(0, 2**63, size=n))
    out, osel, obase, _ = _call(ctx, R, [0, n])
    assert list(obase) == [0, n]
    got = [ids[int(i)] for i in osel[:n]]
    same = np.array([a == b for a, b in zip(got, got[1:])])
    assert same.sum() > n - 20 and np.all(osel[1:n][same] > osel[:n - 1][same])
    _check(ctx, R)


# ---- segments ----------------------------------------------------------------------------------------------

def _lengths(K):
    mix = [0, 1, 64, TILE + 1, 0, 0, 37, 300, 100, 1, 0, 63, 65, 700, 3]
    if K == 1:
        return [TILE + 77]
    if K == 2:
        return [TILE - 30, 95]
    ln = [mix[f % len(mix)] for f in range(K)]
    ln[-1] = 0
    return ln


@pytest.mark.parametrize("K", [1, 2, 64])
def test_segments(ctx, K):
    """K segments of very unequal lengths, empty ones first, in the middle (two adjacent) and last;
    the same few keys stand on both sides of every boundary and no row may cross it. Two rows are out
    of the heap: each falls behind its own segment."""
    ln = _lengths(K)
    base = np.concatenate([[0], np.cumsum(ln)]).astype(np.uint64)
    n = int(base[-1])
    if K > 2:
        assert ln[0] == 0 and ln[-1] == 0 and any(a == 0 and b == 0 for a, b in zip(ln, ln[1:]))
    R = Rows(_random_pairs(n, K, max_len=3), cap=n + 3)
    perm, ob = _check(ctx, R, base=list(base))
    np.testing.assert_array_equal(ob, base)
    for f in range(K):
        seg = perm[int(base[f]):int(base[f + 1])]
        assert np.all((seg >= int(base[f])) & (seg < int(base[f + 1])))
    for i in [2, n - 40]:
        R.cols["key_off"][i] = len(R.heap)
        R.cols["key_len"][i] = 1
        R.bad.add(i)
    _check(ctx, R, base=list(base))


def test_row_base_not_from_zero(ctx):
    """row_base[0] > 0: the rows before it belong to no segment, reach no output and are not counted."""
    R = Rows(_random_pairs(700, 2, max_len=6))
    perm, ob = _check(ctx, R, base=[130, 400, 400, 700])
    assert list(ob) == [0, 270, 270, 570] and perm.min() == 130


# ---- bounds ------------------------------------------------------------------------------------------------

BKEYS = [b"\x01", b"a", b"ab", b"ab\0\0", b"ab\x01", b"abc", b"abd", b"b", b"xyz1", b"xyz2", b"\xfe"]
BOUNDS = {
    "existing": b"abc", "between": b"abcc", "below": b"\x00", "above": b"\xff\xff", "empty": b"",
    "prefix": b"xyz", "trailing_nul": b"ab\0", "longest": b"ab" + b"\0" * (MAXB - 2),
}


def _bound_rows():
    """Every key of BKEYS three to five times under different subsets, shuffled."""
    pairs = []
    for j, k in enumerate(BKEYS):
        pairs += [(k, s) for s in [None, b"s1", b"s2", b"", b"s1x"][:3 + j % 3]]
    rng = np.random.default_rng(23)
    return [pairs[i] for i in rng.permutation(len(pairs))]


def _bound_pages():
    kinds = list(BOUNDS)
    pages = []
    for j, kind in enumerate(kinds):
        b, other = BOUNDS[kind], BOUNDS[kinds[(j + 3) % len(kinds)]]
        pages += [{"from_": b}, {"after": b}, {"until": b},
                  {"from_": b, "until": b"b"}, {"after": b, "until": b"xyz2"},
                  {"from_": other, "until": b}, {"after": other, "until": b}]
    pages += [{"from_": b"abc", "until": b"abc"}, {"after": b"abc", "until": b"abc"}, {"from_": b"b", "until": b"ab"},
              {"after": b"xyz1", "until": b"a"}, {"from_": b"", "until": b""}, {}, None,
              {"from_": b"ab", "until": b"ab\0"}]
    assert len(pages) == 64
    return pages


@pytest.mark.parametrize("keep_ties", [False, True])
@pytest.mark.parametrize("limit", [None, 4])
def test_bounds(ctx, keep_ties, limit):
    """FROM, AFTER, UNTIL, FROM|UNTIL and AFTER|UNTIL, each with a bound equal to an existing key,
    strictly between two keys, below all keys, above all keys, empty, a proper prefix of keys, with a
    trailing \\0, and of 4096 bytes; lo == hi and lo > hi (empty outputs). 64 segments hold the same rows
    and each gets different bounds, in one call; without a limit and with one that cuts inside runs of
    equal key."""
    pairs = _bound_rows()
    m, pages = len(pairs), _bound_pages()
    if limit is not None:
        pages = [dict(g or {}, limit=limit) for g in pages]
    R = Rows(pairs * 64)
    base = [m * f for f in range(65)]
    perm, ob = _check(ctx, R, base=base, pages=pages, keep_ties=keep_ties)
    cnt = np.diff(ob.astype(np.int64))
    if limit is None:
        nkey = lambda pred: sum(1 for k, _ in pairs if pred(k))
        assert cnt[0] == nkey(lambda k: k >= b"abc") and cnt[1] == nkey(lambda k: k > b"abc")
        assert cnt[2] == nkey(lambda k: k < b"abc") and 0 < cnt[2] < cnt[0] + cnt[2] == m
        assert list(cnt[56:61]) == [0, 0, 0, 0, 0] and cnt[61] == m and cnt[62] == m
        assert cnt[63] == nkey(lambda k: k == b"ab")
    elif keep_ties:
        assert cnt.max() > limit  # (a cut moved to its run's end)
    else:
        assert cnt.max() == limit


# ---- limit ---------------------------------------------------------------------------------------------------

def test_limits(ctx):
    """Per-segment limits 0, 1, count - 1, the exact count, above the count and none, exact and with
    KEEP_TIES, over keys without ties and over keys with long runs; a NULL pages equals no bounds and no
    limits."""
    cnt = [300, 300, 300, 300, 300, 300, TILE + 9]
    base = [0] + list(np.cumsum(cnt))
    n = base[-1]
    lim = [0, 1, 299, 300, 301, None, 1000]
    uniq = [(b"%07d" % ((i * 7919) % 100003), None) for i in range(n)]
    runs = _random_pairs(n, 22, max_len=2)
    for pairs in [uniq, runs]:
        R = Rows(pairs)
        for keep in [False, True]:
            _, ob = _check(ctx, R, base=base, pages=[{"limit": v} for v in lim], keep_ties=keep)
            if not keep or pairs is uniq:
                assert list(np.diff(ob.astype(np.int64))) == [0, 1, 299, 300, 300, 300, 1000]
    a = _check(ctx, R, base=base, pages=None)
    b = _check(ctx, R, base=base, pages=[{}] * 7)
    np.testing.assert_array_equal(a[0], b[0])


def test_cut_inside_ties(ctx):
    """Three rows of one key under different subsets, the limit inside them: without the flag exactly
    the limit; with it the output exceeds the limit by exactly the rest of the run. A cut at a run's
    end stays; a run that reaches the segment's end keeps the count; limit 0 keeps nothing."""
    pairs = [(b"a", None), (b"m", b"s2"), (b"b", None), (b"m", None), (b"z", None), (b"m", b"s1"), (b"c", b"q")]
    R = Rows(pairs)
    srt = [(b"a", None), (b"b", None), (b"c", b"q"), (b"m", None), (b"m", b"s1"), (b"m", b"s2"), (b"z", None)]
    for limit, exact, ties in [(4, 4, 6), (5, 5, 6), (6, 6, 6), (3, 3, 3), (0, 0, 0), (7, 7, 7), (1, 1, 1)]:
        perm, ob = _check(ctx, R, pages=[{"limit": limit}], keep_ties=False)
        assert list(ob) == [0, exact] and [pairs[i] for i in perm] == srt[:exact]
        perm, ob = _check(ctx, R, pages=[{"limit": limit}], keep_ties=True)
        assert list(ob) == [0, ties] and [pairs[i] for i in perm] == srt[:ties]
    tail = Rows([p for p in pairs if p[0] != b"z"])  # (the run of "m" is now the segment's end)
    assert list(_check(ctx, tail, pages=[{"limit": 4}], keep_ties=True)[1]) == [0, 6]
    # a long run across several tiles, the cut in its middle, behind a bound
    big = Rows([(b"a", None)] * 100 + [(b"mm", b"s%d" % (i % 3)) for i in range(3 * TILE)] + [(b"z", None)] * 50)
    assert list(_check(ctx, big, pages=[{"after": b"a", "limit": TILE}], keep_ties=True)[1]) == [0, 3 * TILE]
    assert list(_check(ctx, big, pages=[{"after": b"a", "limit": TILE}], keep_ties=False)[1]) == [0, TILE]


# ---- untouched memory, argument checks, determinism --------------------------------------------------------------

@pytest.mark.parametrize("base", ["past_cap", "decreasing"])
def test_invalid_row_base(ctx, base):
    """row_base[nseg] = rows_cap + 1, and a row_base that decreases: out_base is all 0, totals are 0 and
    nothing else is written."""
    n = 500
    R = Rows(_random_pairs(n, 1))
    rb = [0, 200, n + 1] if base == "past_cap" else [0, 300, 200, n]
    out, osel, obase, tot = _call(ctx, R, rb, pages=[{"from_": b"a"}] * (len(rb) - 1))
    assert not obase.any() and not tot.any()
    g_rows, g_sel, _ = _guards(n, len(rb) - 1)
    np.testing.assert_array_equal(osel, g_sel)
    for k in SRC:
        np.testing.assert_array_equal(out[k], g_rows[k], err_msg=k)


def test_untouched_tails(ctx):
    """Entries of out_rows and out_sel_idx at or beyond out_base[nseg] keep their sentinel when bounds
    and limits keep a few rows of many (checked by _check), and out_sel_idx may be absent."""
    R = Rows(_random_pairs(900, 3, max_len=4), cap=1000)
    _, ob = _check(ctx, R, base=[0, 450, 900], pages=[{"from_": b"a", "limit": 5}, {"until": b"a\x80", "limit": 9}])
    assert list(ob) == [0, 5, 14]
    out, osel, obase, _ = _call(ctx, R, [0, 450, 900], pages=[{"limit": 5}, {"limit": 9}], sel=False)
    assert osel is None and list(obase) == [0, 5, 14] and np.all(out["change"][14:] == _guards(1000, 2)[0]["change"][14:])


def test_argument_checks(ctx):
    from _gpu import drp_amd
    n = 100
    R = Rows(_random_pairs(n, 1))
    rows = {k: _up(v) for k, v in R.cols.items()}
    out = {k: _up(np.zeros_like(v)) for k, v in R.cols.items()}
    base, obase = _up(np.array([0, n], np.uint64)), _up(np.zeros(2, np.uint64))
    sel, heap = _up(np.arange(n, dtype=np.uint64)), _up(R.heap)

    def bad(**kw):
        a = dict(heap_t=heap, rows=rows, row_base_t=base, nseg=1, rows_cap=n, out_rows=out, out_base_t=obase)
        a.update(kw)
        with pytest.raises(drp_amd.DrpError) as e:
            ctx.order_keys_device(**a)
        assert e.value.rc == drp_amd.DRP_E_INVAL, kw

    bad(nseg=0)
    bad(nseg=drp_amd.FANOUT_MAX + 1)
    bad(rows=None)
    bad(row_base_t=None)
    bad(out_rows=None)
    bad(out_base_t=None)
    bad(out_sel_idx_t=sel)  # (without sel_idx)
    bad(out_rows=dict(out, change=rows["change"]))  # in place
    bad(rows=dict(rows, key_len=None))
    bad(flags=2)
    bad(flags=0x80000001)
    bad(rows_cap=2**32)
    bad(pages=[drp_amd.make_key_page(flags=8)])
    bad(pages=[drp_amd.make_key_page(from_=b"a", after=b"b")])
    bad(pages=[drp_amd.make_key_page(until=bytes(MAXB + 1))])
    ctx.order_keys_device(heap, rows, base, 1, n, out, obase,
                          pages=[drp_amd.make_key_page(until=bytes(MAXB))])  # (a bound of the greatest length is accepted)
    assert list(_down(obase)) == [0, sum(1 for k in R.keys if k < bytes(MAXB))]
    ctx.order_keys_device(heap, rows, base, 1, n, out, obase)  # (the same arguments as they stand are accepted)
    assert list(_down(obase)) == [0, n]


def test_deterministic(ctx):
    n = 3 * TILE + 11
    R = Rows(_random_pairs(n, 6, max_len=3))
    base = [0, 1000, 1000, 2 * TILE, n]
    pages = [{"limit": 5000}, {"limit": 7}, {"from_": b"a", "limit": 3000}, {"until": b"b"}]
    a = _call(ctx, R, base, pages=pages, keep_ties=True)
    b = _call(ctx, R, base, pages=pages, keep_ties=True)
    for k in SRC:
        np.testing.assert_array_equal(a[0][k], b[0][k], err_msg=k)
    for x, y in zip(a[1:], b[1:]):
        np.testing.assert_array_equal(x, y)


def test_order_device_unchanged(ctx):
    """drp_order_device on the same rows before and after a key-order call on the same ctx (the two
    share scratch and pass kernels): the stable argsort of `change` both times, with a limit and
    KEEP_TIES."""
    n = TILE + 500
    change = np.random.default_rng(8).integers(0, 50, size=n).astype(np.uint64)
    R = Rows(_random_pairs(n, 9, max_len=5), change=change)
    base = [0, 700, 700, n]

    def by_change():
        d_rows = {k: _up(v) for k, v in R.cols.items()}
        d_out = {k: _up(v) for k, v in _guards(n, 3)[0].items()}
        d_sel, d_osel = _up(np.arange(n, dtype=np.uint64)), _up(_guards(n, 3)[1])
        d_base, d_obase = _up(np.asarray(base, np.uint64)), _up(_guards(n, 3)[2])
        ctx.order_device(d_rows, d_base, 3, n, d_out, d_obase, limit=[100, 5, None], keep_ties=True, sel_idx_t=d_sel,
                         out_sel_idx_t=d_osel)
        return _down(d_osel), _down(d_obase), _down(d_out["change"])

    want, ob = [], [0]
    for f, lim in enumerate([100, 5, None]):
        lo, hi = base[f], base[f + 1]
        order = lo + np.argsort(change[lo:hi], kind="stable")
        kept = len(order) if lim is None else min(len(order), lim)
        while 0 < kept < len(order) and change[order[kept]] == change[order[kept - 1]]:
            kept += 1
        want += list(order[:kept])
        ob.append(ob[-1] + kept)
    before = by_change()
    _check(ctx, R, base=base, pages=[{"limit": 50}, None, {"from_": b"a"}], keep_ties=True)
    after = by_change()
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)
    assert list(before[1]) == ob
    np.testing.assert_array_equal(before[0][:ob[-1]], np.array(want, np.uint64))
    np.testing.assert_array_equal(before[2][:ob[-1]], change[want])


# ---- end to end through the store ----------------------------------------------------------------------


def _decode(wire):
    """The Changes of a wire, in wire order, by the oracle."""
    if not wire:
        return []
    ref = O.decode_batch(wire)
    n = ref["nframes"]
    assert ref["err_code"] == 0 and ref["consumed"] == len(wire) and np.all(ref["type"][:n] == 1)
    return [change_at(wire, ref, i) for i in range(n)]


def _content():
    """About 300 identities over three subsets (absent, "s1", "s2"); keys of 2 to 30 bytes, most under
    "k/", many present under two or three subsets, some a prefix of others."""
    rng = np.random.default_rng(31)
    rows, seen = [], set()
    while len(rows) < 300:
        j = int(rng.integers(0, 200))
        stem = b"k/" if j % 5 else b"other/"
        key = stem + (b"%d" % j) * (1 + j % 4) + (b"\0" if j % 11 == 0 else b"")
        sub = [None, b"s1", b"s2"][int(rng.integers(0, 3))]
        if (sub, key) in seen:
            continue
        seen.add((sub, key))
        i = len(rows)
        rows.append((key, sub, 10 + i % 37, i % 100, i % 7, b"v%d" % i if i % 3 else None))
    return rows


@pytest.fixture(scope="module")
def store(ctx):
    import torch
    from _gpu import drp_amd
    batch = _content()
    wire = b"".join(S.frame(S.change_payload(k, ch, fr, to, value=v, subset=sub)) for k, sub, ch, fr, to, v in batch)
    st = drp_amd.Store(ctx, 400, 1 << 16)
    g = ctx.decode_staged(wire)
    n = g["nframes"]
    assert n == len(batch)
    cols = {k: _up(g[k][:n]) for k in ["payload_off", "payload_len", "type", "flags"] + O.COLS32 + O.COLS64}
    st.merge_device(torch.from_numpy(np.frombuffer(wire, np.uint8).copy()).to("cuda:0"), cols, n)
    info = st.query()
    assert info.rows == 300 and not info.refused
    return st


def _listing(spec):
    """The model's full listing under a filter spec: the store's Changes that pass, sorted."""
    rows = []
    for k, sub, ch, fr, to, v in _content():
        if "subset" in spec and sub != spec["subset"]:
            continue
        if spec.get("subset_none") and sub is not None:
            continue
        if "key_prefix" in spec and not k.startswith(spec["key_prefix"]):
            continue
        if "change_range" in spec and not spec["change_range"][0] <= ch <= spec["change_range"][1]:
            continue
        rows.append(Change(sub is not None, sub or b"", k, ch, fr, to, v is not None, v or b""))
    return sorted(rows, key=lambda c: (c.key, c.has, c.subset))


def _page_through(store, specs, limit):
    """The paging loop over all specs at once: after = last_key until every page is empty. Returns the
    decoded pages per spec, concatenated, and the page sizes."""
    from _gpu import drp_amd
    K = len(specs)
    after, got, sizes, rounds = [None] * K, [[] for _ in range(K)], [[] for _ in range(K)], 0
    while True:
        rounds += 1
        assert rounds <= 200
        pages = [drp_amd.make_key_page(after=after[f], limit=limit) for f in range(K)]
        res = store.list_keys([drp_amd.make_filter(**s) if s else None for s in specs], pages, keep_ties=True)
        if all(sent == 0 for _, sent, _ in res):
            assert all(w == b"" and last is None for w, _, last in res)
            break
        for f, (w, sent, last) in enumerate(res):
            if sent:
                rows = _decode(w)
                assert len(rows) == sent and rows[-1].key == last
                assert after[f] is None or (last > after[f] and rows[0].key > after[f])  # every page makes progress
                got[f] += rows
                sizes[f].append(sent)
                after[f] = last
    return got, sizes


def test_store_list_keys_paging(ctx, store):
    """Store.list_keys under a subset filter plus key_prefix, limit=7, keep_ties=True: the paging loop
    with after = last_key runs until a page is empty; the concatenation of the decoded pages equals
    the model's full sorted listing, no row twice, none missing."""
    spec = {"subset": b"s1", "key_prefix": b"k/"}
    got, sizes = _page_through(store, [spec], 7)
    want = _listing(spec)
    assert len(want) > 50 and got[0] == want
    assert max(collections.Counter(got[0]).values()) == 1
    assert all(s == 7 for s in sizes[0][:-1])  # (one subset: no two rows share a key, no page passes the limit)


def test_store_list_keys_three_filters(ctx, store):
    """The same with K = 3 filters in one call: a subset plus a prefix, everything (one key under up to
    three subsets: KEEP_TIES pages pass the limit, and the resume loses no row), and a version-bounded
    listing of the rows without a subset."""
    specs = [{"subset": b"s2", "key_prefix": b"k/1"}, {}, {"subset_none": True, "change_range": (20, 40)}]
    got, sizes = _page_through(store, specs, 7)
    for f, spec in enumerate(specs):
        want = _listing(spec)
        assert len(want) > 5 and got[f] == want, f
        assert max(collections.Counter(got[f]).values()) == 1, f
    assert len(got[1]) == 300 and max(sizes[1]) > 7 and min(sizes[1][:-1]) >= 7
    # one page without a limit, bounded on both sides, is the model's slice
    from _gpu import drp_amd
    res = store.list_keys([None], [drp_amd.make_key_page(from_=b"k/2", until=b"k/5")], keep_ties=False)
    want = [c for c in _listing({}) if b"k/2" <= c.key < b"k/5"]
    assert _decode(res[0][0]) == want and res[0][1] == len(want) > 20 and res[0][2] == want[-1].key
