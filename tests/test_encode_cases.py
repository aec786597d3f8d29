"""CPU checks of tests/_encode.py, the case builders behind tests/test_gpu_encode.py: every case
reaches the state of csrc/drp_encode.hip it is named for (a block with exactly ENC_FMAX frames and
one above it, a frame over several output blocks, every varint width, dense or sparse blocks around
the rows it is about), read from the oracle's frame offsets with frames_touching, the restatement of
enc_write_os's f1 - f0. An edit to a builder that loses a geometry fails here, not silently on the
GPU."""
import os
import re

import numpy as np
import pytest

import _encode as E
import _oracle as O
import _streams as S

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dat-replication-protocol_amd",
                   "csrc", "drp_encode.hip")
SHIFTS = range(16)


def test_constants_match_the_kernel():
    text = open(SRC).read()
    assert int(re.search(r"#define DRP_ENC_BS (\d+)", text).group(1)) == E.ENC_BS
    assert int(re.search(r"\bENC_FMAX = (\d+)", text).group(1)) == E.ENC_FMAX
    assert re.search(r"constexpr uint32_t ENC_BS = DRP_ENC_BS\b", text)
    assert re.search(r"if \(n < 128\)", text), "wave_copy's vector path starts at 128 bytes (WAVE_LENS)"
    assert int(re.search(r"SCAN_BLK = (\d+)", text).group(1)) == 1024


def test_frames_touching_by_hand():
    """Three frames of 65536, 10 and 65526 bytes. Unshifted: block 0 holds frame 0 and the frame that
    starts exactly at its end (2 frames), block 1 frames 1 and 2. Shifted by one: block 0 ends inside
    frame 0, which the next block's first byte belongs to (1 frame); block 1 holds all three; block 2
    the last byte."""
    fo = np.array([0, 65536, 65546, 131072], np.uint64)
    assert E.frames_touching(fo, 0).tolist() == [2, 2]
    assert E.frames_touching(fo, 1).tolist() == [1, 3, 1]
    assert E.frames_touching(np.array([0, 10], np.uint64), 15).tolist() == [1]
    assert list(E.block_of(fo, 0, 1)) == [1] and list(E.block_of(fo, 1, 0)) == [0, 1]


def test_frame_off_is_arithmetic():
    """The oracle's frame offsets equal header + type + payload summed from the field lengths."""
    c = E.mixed_short(500)
    fl = c.cols["flags"]
    tot = []
    for i in range(c.n):
        p = 1 + E.vlen(int(c.cols["key_len"][i])) + int(c.cols["key_len"][i])
        p += sum(1 + E.vlen(int(c.cols[k][i])) for k in ("change", "from", "to"))
        for bit, k in ((E.F_SUBSET, "subset_len"), (E.F_VALUE, "value_len")):
            if fl[i] & bit:
                p += 1 + E.vlen(int(c.cols[k][i])) + int(c.cols[k][i])
        tot.append(E.vlen(p + 1) + 1 + p)
    np.testing.assert_array_equal(c.frame_off, np.concatenate([[0], np.cumsum(tot)]).astype(np.uint64))
    assert set(fl.tolist()) == {0, 1, 2, 3}


@pytest.mark.parametrize("n", E.SMALL_COUNTS)
def test_row_counts(n):
    c = E.mixed_short(n, seed=10 + n)
    assert c.n == n and len(c.frame_off) == n + 1 and int(c.frame_off[-1]) == len(c.exp)


def test_past_one_scan_round():
    c = E.past_one_scan_round()
    assert c.n == (1 << 20) + 2 and (c.n + 1023) // 1024 == 1025  # 1025 block sums: a second scan round
    np.testing.assert_array_equal(c.frame_off[:c.n], np.arange(c.n, dtype=np.uint64) * 10)
    last = S.frame(S.change_payload(c.heap[:5].tobytes(), 1 << 40, 300, 7, value=c.heap[5:42].tobytes()))
    assert len(last) == 60 and len(c.exp) == 10 * ((1 << 20) + 1) + 60 and int(c.frame_off[-1]) == len(c.exp)
    assert c.exp[-60:] == last and c.exp[-70:-60] == S.frame(S.change_payload(b"", 0, 0, 0))


def test_varint_widths():
    c = E.varint_widths()
    fo, exp = c.frame_off, c.exp
    d = O.decode_batch(exp, cap=c.n + 2)
    widths = set()
    for row, p1 in c.rows["header"].items():
        assert int(d["payload_len"][row]) + 1 == p1
        w = int(d["payload_off"][row]) - int(fo[row]) - 1
        assert exp[int(fo[row]):int(fo[row]) + w] == S.varint(p1)
        widths.add((p1, w))
    assert widths == {(127, 1), (128, 2), (16383, 2), (16384, 3), ((1 << 21) - 1, 3), (1 << 21, 4)}
    seen = set()
    for row, (field, ln) in c.rows["prefix"].items():
        assert int(c.cols[field + "_len"][row]) == ln and c.cols["flags"][row] == 3
        at = int(d["payload_off"][row]) + int(d[field + "_off"][row])  # the field's first byte in the wire
        w = len(S.varint(ln))
        assert exp[at - w:at] == S.varint(ln) and int(d[field + "_len"][row]) == ln
        seen.add((field, w))
    assert seen == {(f, w) for f in ("key", "subset", "value") for w in (1, 2, 3, 4)}
    # the long rows' headers: four bytes too (a payload of 2^21 and more)
    assert sum(int(d["payload_off"][r]) - int(fo[r]) - 1 == 4 for r in c.rows["prefix"]) == 3
    # five bytes from 2^28 on, by arithmetic: the prefix of a 2^28-byte value and its frame's header
    assert len(S.varint((1 << 28) - 1)) == 4 and len(S.varint(1 << 28)) == 5 and E.vlen(1 << 28) == 5
    assert len(S.varint((1 << 28) + 30)) == 5


def _split_payload(case, row):
    c, h = case.cols, case.heap
    cut = lambda name: h[int(c[name + "_off"][row]):int(c[name + "_off"][row]) + int(c[name + "_len"][row])].tobytes()
    fl = int(c["flags"][row])
    return S.frame(S.change_payload(cut("key"), int(c["change"][row]), int(c["from"][row]), int(c["to"][row]),
                                    value=cut("value") if fl & E.F_VALUE else None,
                                    subset=cut("subset") if fl & E.F_SUBSET else None))


@pytest.mark.parametrize("mis", [0, 1, 15])
def test_long_fields(mis):
    c = E.long_fields(mis)
    fo, exp = c.frame_off, c.exp
    assert sorted(c.rows["long"].values()) == sorted(E.LONG_ROWS)
    for row, (field, ln) in c.rows["long"].items():
        assert int(c.cols[field + "_len"][row]) == ln and int(c.cols[field + "_off"][row]) % 16 == mis
    # the wire, a second time: the Python statement of the framing, row by row
    for row in range(c.n):
        assert exp[int(fo[row]):int(fo[row + 1])] == _split_payload(c, row), row
    big = max(c.rows["long"], key=lambda r: c.rows["long"][r][1])
    for shift in SHIFTS:
        t = E.frames_touching(fo, shift)
        assert t.max() <= E.ENC_FMAX  # every block goes to the block writer
        for row in c.rows["long"]:
            assert len(E.block_of(fo, shift, row)) >= 2  # every long frame spans blocks
        blocks = E.block_of(fo, shift, big)
        assert len(blocks) >= 2 + 3 and (t[blocks[1]:blocks[-1]] == 1).all()  # three whole blocks or more: one frame each
        # frame-relative offsets past 16 bits and past 2^21 inside one frame
        assert int(fo[big + 1] - fo[big]) > (1 << 21)


@pytest.mark.parametrize("where", ["behind", "before"])
def test_long_fields_next_to_dense_blocks(where):
    """300 ten-byte frames directly before (the long row lies behind them) or after every long row:
    the block holding that end of the long frame is dense, the frame's other blocks are not."""
    kw = {"tiny_behind": 300} if where == "behind" else {"tiny_before": 300}
    c = E.long_fields(3, **kw)
    fo = c.frame_off
    for shift in SHIFTS:
        t = E.frames_touching(fo, shift)
        for row in c.rows["long"]:
            blocks = E.block_of(fo, shift, row)
            shared = blocks[0] if where == "behind" else blocks[-1]
            assert t[shared] > E.ENC_FMAX, (shift, row)
            assert (t[blocks[1]:blocks[-1]] <= E.ENC_FMAX).all() and len(blocks) >= 2


def test_block_switch():
    c = E.block_switch()
    sizes = (c.frame_off[1:] - c.frame_off[:-1]).astype(np.int64)
    np.testing.assert_array_equal(sizes, c.rows["size"])
    assert set(sizes.tolist()) == set(E.SWITCH_SIZES) and c.n == 700 * 25
    for shift in SHIFTS:
        t = E.frames_touching(c.frame_off, shift)
        assert (t == E.ENC_FMAX).any() and (t > E.ENC_FMAX).any() and (t < E.ENC_FMAX).any(), shift
        assert E.ENC_FMAX + 1 in t  # the first count the LDS layout does not hold


def test_chunk_edges():
    dense, sparse = E.chunk_edges(False), E.chunk_edges(True)
    combos = set()
    for c in (dense, sparse):
        r = c.rows["edge"]
        assert len(r) == 8 * 8 * 8 * 4 * 2
        got = set(zip(*(c.cols[k][r].tolist() for k in ("key_len", "subset_len", "value_len", "flags")),
                      (c.cols["change"][r] >> np.uint64(63)).tolist()))
        assert len(got) == len(r)
        combos |= got
    assert combos == {(k, s, v, f, w) for k in E.EDGE_LENS for s in E.EDGE_LENS for v in E.EDGE_LENS
                      for f in range(4) for w in range(2)}
    assert (np.diff(sparse.frame_off.astype(np.int64))[1::2] > 1030).all()
    for shift in SHIFTS:
        assert E.frames_touching(dense.frame_off, shift).min() > E.ENC_FMAX
        t = E.frames_touching(sparse.frame_off, shift)
        assert t.max() <= E.ENC_FMAX and t.max() >= 100, (shift, t.max())


@pytest.mark.parametrize("mis", [0, 9])
def test_wave_copy_rows(mis):
    c = E.wave_copy_rows(mis)
    assert sorted(c.rows["wave"].values()) == sorted((f, n) for f in ("key", "subset", "value") for n in E.WAVE_LENS)
    for row, (field, ln) in c.rows["wave"].items():
        assert int(c.cols[field + "_len"][row]) == ln and int(c.cols[field + "_off"][row]) % 16 == mis
    dst = set()
    d = O.decode_batch(c.exp, cap=c.n + 2)
    for shift in SHIFTS:
        t = E.frames_touching(c.frame_off, shift)
        assert t.min() > E.ENC_FMAX  # every block dense: the per-frame writer writes every row
        for row, (field, ln) in c.rows["wave"].items():
            dst.add((ln, (int(d["payload_off"][row]) + int(d[field + "_off"][row]) + shift) % 16))
    # every destination alignment of every length (with every source alignment: `mis` is free)
    assert dst == {(n, a) for n in E.WAVE_LENS for a in range(16)}
