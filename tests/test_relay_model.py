"""CPU: the expected side the relay-family GPU tests share (_relay.mask, _relay.winners) gives, over
one hand-built wire, exactly the rows written out here by hand."""
import numpy as np
import pytest

import _oracle as O
import _relay as R
import _streams as S

# row: (key, subset or None, change); from = row, to = row + 1, a value on the odd rows
ROWS = [
    (b"a/1", None, 5),    # 0: absent subset; beaten by row 4
    (b"a/2", b"s", 10),   # 1
    (b"a/", b"", 15),     # 2: the key is the prefix "a/" itself; the subset is present and empty
    (b"b/1", b"t", 20),   # 3: beaten by row 7 (equal change, the later row)
    (b"a/1", None, 25),   # 4: row 0's identity with a greater change
    (b"a/1", b"s", 30),   # 5: row 0's key under a subset: another identity
    (b"ab", None, 20),    # 6: shares "a" with the others, not "a/"
    (b"b/1", b"t", 20),   # 7: row 3's identity and change
]
WIRE = b"".join(S.frame(S.change_payload(k, ch, r, r + 1, value=b"v%d" % r if r % 2 else None, subset=sub))
                for r, (k, sub, ch) in enumerate(ROWS))

MASKS = [
    ({}, [0, 1, 2, 3, 4, 5, 6, 7]),
    ({"change_range": (10, 25)}, [1, 2, 3, 4, 6, 7]),
    ({"subset": b"s"}, [1, 5]),
    ({"subset": b""}, [2]),
    ({"subset_none": True}, [0, 4, 6]),
    ({"key_prefix": b"a/"}, [0, 1, 2, 4, 5]),
    ({"subset_none": True, "key_prefix": b"a/", "change_range": (10, 25)}, [4]),
]
WINNERS = [
    ({}, [1, 2, 4, 5, 6, 7]),
    ({"change_range": (0, 12)}, [0, 1]),  # the snapshot at 12: row 0 holds its identity, row 4 is not in it
    ({"subset_none": True}, [4, 6]),
    ({"subset": b"t"}, [7]),
]


@pytest.fixture(scope="module")
def ref():
    r = O.decode_batch(WIRE)
    assert r["nframes"] == len(ROWS) and r["err_code"] == 0 and r["consumed"] == len(WIRE)
    return r


@pytest.mark.parametrize("spec,want", MASKS, ids=[",".join(s) or "all" for s, _ in MASKS])
def test_mask(ref, spec, want):
    for wire in (WIRE, np.frombuffer(WIRE, np.uint8)):
        assert np.flatnonzero(R.mask(wire, ref, len(ROWS), spec)).tolist() == want
    assert np.flatnonzero(R.mask(WIRE, ref, 5, spec)).tolist() == [i for i in want if i < 5]  # rows [0, n) only


@pytest.mark.parametrize("spec,want", WINNERS, ids=[",".join(s) or "all" for s, _ in WINNERS])
def test_winners(ref, spec, want):
    idx, best = R.winners(WIRE, ref, np.flatnonzero(R.mask(WIRE, ref, len(ROWS), spec)))
    assert idx.dtype == np.int64 and idx.tolist() == want
    ident = lambda r: (ROWS[r][1] is not None, ROWS[r][1] or b"", ROWS[r][0])
    assert best == {ident(r): (ROWS[r][2], r) for r in want}
    rows, changes = R.wire_winners(WIRE, spec)
    assert rows == want
    assert changes == [R.Change(*ident(r), ROWS[r][2], r, r + 1, bool(r % 2), b"v%d" % r if r % 2 else b"") for r in want]


def test_check_decoded_names_the_row_and_field(ref):
    cols = R.rows(ref, np.array([1, 2, 5]))
    R.check_decoded(O.encode_changes(WIRE, cols), WIRE, cols)
    other = R.rows(ref, np.array([1, 2, 4]))  # (row 4 for row 5: the key stands, the subset does not)
    other["change"][2], other["from"][2], other["to"][2] = cols["change"][2], cols["from"][2], cols["to"][2]
    other["flags"][2] = cols["flags"][2]
    with pytest.raises(AssertionError, match="row 2, subset"):
        R.check_decoded(O.encode_changes(WIRE, cols), WIRE, other)


def test_rows_are_absolute_and_masked(ref):
    cols = R.rows(ref, np.array([2, 5]), base=100)
    assert sorted(cols) == sorted(R.SRC_KEYS)
    assert [R.field_bytes(b"\0" * 100 + WIRE, cols, "key", i) for i in range(2)] == [b"a/", b"a/1"]
    assert R.field_bytes(b"\0" * 100 + WIRE, cols, "value", 1) == b"v5" and cols["flags"].tolist() == [1, 3]
    assert [cols[k].dtype for k in R.SRC_KEYS] == [np.dtype(R.dtype(k)) for k in R.SRC_KEYS]
