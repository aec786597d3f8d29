"""GPU: drp_decode_batch into caller-owned DEVICE columns (decode_batch_device_out in
csrc/drp_api.hip). The bindings never take this path (Ctx.decode_batch passes host columns, the
addon stages and fetches), so the calls here go through ctx.L.drp_decode_batch with torch device
tensors as the columns. Every column, n_frames, err_* and every Carry field are compared with the
oracle's decode of the same batch; every column has one row more than `cap` and is filled with
0xAB beforehand, and nothing may be written at or past min(cap, rows)."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import _change_model as M
import _oracle as O
import _streams as S

pytestmark = pytest.mark.gpu

DT = {"payload_off": np.uint64, "payload_len": np.uint32, "type": np.uint8, "flags": np.uint8, "key_hash": np.uint64,
      **{k: np.uint32 for k in O.COLS32}, **{k: np.uint64 for k in O.COLS64}}
FRAME_COLS = ["payload_off", "payload_len", "type"]
CHANGE_COLS = O.COLS32 + O.COLS64 + ["flags"]
FILL = 0xAB
T_CHANGE, T_BLOB, F_CONT, F_PARTIAL = 1, 2, 0x40, 0x80
TAIL_NONE, TAIL_HEADER, TAIL_CHANGE, TAIL_BLOB = 0, 1, 2, 3
KEY_CLASS = 0x30  # DRP_F_KEY_ASCII | DRP_F_KEY_UTF8: set by the key pass only

C2 = S.c2_stream(300, seed=5).tobytes()  # 300 canonical 86-byte Change frames
C3 = S.c3_stream(random.Random(3), 3, frames_per_unit=40, blob_len=3000)  # 3 x (40 Changes + a blob)
MISSING = S.frame(M.fields(to=None))  # a Change without its required `to`
BAD = C2[:86 * 20] + MISSING + C2[86 * 20:86 * 60]  # the malformed Change in the middle


@pytest.fixture(scope="module")
def ctx():
    from _gpu import drp_amd
    c = drp_amd.Ctx(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _ref(w, brem):
    """The oracle's decode of the whole chain (its capacity is never short); shared, never changed."""
    r = O.decode_batch(w, blob_remaining=brem, cap=len(w) // 2 + 3)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def _frame_bytes(w, r):
    """Carry.frame_bytes: the cut Change frame's header, id and payload bytes (0 for every other
    tail), read from the wire at the oracle's `consumed`."""
    if r["tail"] != TAIL_CHANGE:
        return 0
    at, n, sh = r["consumed"], 0, 0
    while True:
        n |= (w[at] & 0x7F) << sh
        sh += 7
        at += 1
        if w[at - 1] < 0x80:
            return at - r["consumed"] + n


def _wire(kind, w):
    """(pointer, object that keeps the bytes alive) for the three ways a batch can arrive."""
    import torch
    a = np.frombuffer(w, np.uint8) if len(w) else np.zeros(16, np.uint8)
    if kind == "host":  # staged through in_stage
        return C.c_void_p(a.ctypes.data), a
    shift = 1 if kind == "device+1" else 0  # +1: a device pointer that is not 16-byte aligned (staged too)
    t = torch.zeros(a.size + shift, dtype=torch.uint8, device="cuda:0")
    t[shift:] = torch.from_numpy(a.copy())
    assert t.data_ptr() % 16 == 0  # "device": decoded in place
    return C.c_void_p(t.data_ptr() + shift), t


def _decode(ctx, kind, w, brem, cap, key_hash=False):
    """One drp_decode_batch into device columns of cap + 1 rows filled with 0xAB: (rc, the columns
    as host arrays, n_frames, err_frame, err_code, err_detail, carry)."""
    import torch

    from _gpu import drp_amd
    names = FRAME_COLS + CHANGE_COLS + (["key_hash"] if key_hash else [])
    cols = {k: torch.full(((cap + 1) * np.dtype(DT[k]).itemsize,), FILL, dtype=torch.uint8, device="cuda:0")
            for k in names}
    ptr, keep = _wire(kind, w)
    torch.cuda.synchronize()  # (libdrp runs on a stream of its own)
    fr, co = drp_amd._structs(cols, lambda t: C.c_void_p(t.data_ptr()))
    carry = drp_amd.Carry(brem, 0, 0, 0, 0)
    nf, ef, ec, ed = C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_uint32()
    rc = ctx.L.drp_decode_batch(ctx.h, ptr, len(w), C.byref(carry), C.byref(fr), C.byref(co), cap, C.byref(nf),
                                C.byref(ef), C.byref(ec), C.byref(ed))
    assert ctx.L.drp_synchronize(ctx.h) == 0
    del keep
    host = {k: v.cpu().numpy().view(DT[k]) for k, v in cols.items()}
    return rc, host, nf.value, ef.value, ec.value, ed.value, carry


def _filled(k, n):
    return np.full(n * np.dtype(DT[k]).itemsize, FILL, np.uint8).view(DT[k])


def _check(got, w, brem, cap, label, key_ref=None):
    """A call's outputs against the oracle's decode of (w, brem): the return code from the
    capacity, the rows below min(cap, rows), the guard cells from there on, counts, error and
    carry. key_ref: a decode_batch(key_hash=True) into host columns, for key_hash and the key
    class flags."""
    from _gpu import drp_amd
    rc, host, nf, ef, ec, ed, carry = got
    r = _ref(w, brem)
    rows = len(r["type"])  # delivered frames, plus the malformed Change
    if not r["err_code"]:  # (the frames behind a malformed Change take rows too: its test checks rc)
        assert rc == (drp_amd.DRP_OK if cap >= rows else drp_amd.DRP_E_CAPACITY), (label, rc, cap, rows)
    assert nf == r["nframes"], (label, "n_frames", nf, r["nframes"])
    assert (ec, ed) == (r["err_code"], r["err_detail"]), (label, "err", ec, ed, r["err_code"], r["err_detail"])
    assert ef == (r["err_frame"] if r["err_code"] else 2**64 - 1), (label, "err_frame", ef, r["err_frame"])
    assert (carry.blob_remaining, carry.consumed, carry.tail_kind) == (r["blob_remaining"], r["consumed"], r["tail"]), \
        (label, "carry", carry.blob_remaining, carry.consumed, carry.tail_kind, r["blob_remaining"], r["consumed"],
         r["tail"])
    assert carry.frame_bytes == _frame_bytes(w, r), (label, "frame_bytes", carry.frame_bytes)
    m = min(cap, rows)
    for k in FRAME_COLS:
        np.testing.assert_array_equal(host[k][:m], r[k][:m], err_msg=f"{label}:{k}")
    ch = (r["type"][:m] & 0x3F) == T_CHANGE
    for k in CHANGE_COLS:
        g, want = host[k][:m][ch], r[k][:m][ch]
        if key_ref is not None and k == "flags":  # the key pass adds the key's class to the flags
            want = key_ref[k][:m][ch]
            np.testing.assert_array_equal(want & (0xFF ^ KEY_CLASS), r[k][:m][ch], err_msg=f"{label}:flags (host)")
        np.testing.assert_array_equal(g, want, err_msg=f"{label}:{k}")
    if key_ref is not None:
        np.testing.assert_array_equal(host["key_hash"][:m][ch], key_ref["key_hash"][:m][ch], err_msg=f"{label}:key_hash")
        # rows that are no Changes (blobs, the carried blob's row 0) are not written
        np.testing.assert_array_equal(host["key_hash"][:m][~ch], _filled("key_hash", int((~ch).sum())),
                                      err_msg=f"{label}:key_hash of the other rows")
    return m, host


def _check_guard(host, m, label):
    for k, v in host.items():
        np.testing.assert_array_equal(v[m:], _filled(k, len(v) - m), err_msg=f"{label}:{k} written at or past row {m}")


@pytest.mark.parametrize("kind", ["device", "device+1", "host"])
@pytest.mark.parametrize("name", ["c2", "c3", "c3.cut.blob", "c3.cut.change", "c3.cut.header"])
def test_wire_kinds(ctx, kind, name):
    """A device tensor decoded in place, the same bytes one byte off alignment and a host array
    (both staged): whole batches and the three kinds of cut tail."""
    w = {"c2": C2, "c3": C3,
         "c3.cut.blob": C3[:-1000],  # inside the last blob's payload
         "c3.cut.change": C3[:86 * 40 + 3003 + 86 * 7 + 30],  # inside a Change of the second unit
         "c3.cut.header": C3[:86 * 40 + 1]}[name]  # after the first byte of a blob's two-byte length
    r = _ref(w, 0)
    assert r["tail"] == {"c2": TAIL_NONE, "c3": TAIL_NONE, "c3.cut.blob": TAIL_BLOB, "c3.cut.change": TAIL_CHANGE,
                         "c3.cut.header": TAIL_HEADER}[name]
    cap = len(r["type"]) + 2
    m, host = _check(_decode(ctx, kind, w, 0, cap), w, 0, cap, (kind, name))
    _check_guard(host, m, (kind, name))


def _carried(brem, body):
    """`brem` bytes of a blob opened in an earlier batch, then `body`."""
    return bytes((11 * i + 5) & 0xFF for i in range(brem)) + body


CARRIED = {"aligned": (4096, C2), "unaligned": (4099, C2), "c3.unaligned": (1001, C3[:-1000]),
           "all": (5000, b""), "more": (5007, b"")}


@pytest.mark.parametrize("kind", ["device", "device+1", "host"])
@pytest.mark.parametrize("case", list(CARRIED))
def test_carried_blob(ctx, kind, case):
    """carry.blob_remaining on entry: row 0 is the continuation (BLOB | CONT, PARTIAL with it when
    the blob goes on past the batch), the GPU's rows start at row 1, and the carry is right for the
    two early exits (the batch is all continuation: brem == n, brem > n) and for the decode behind
    the blob's end at a 16-byte aligned offset and at an odd one."""
    brem, body = CARRIED[case]
    n = len(body) + min(brem, 5000)
    w = _carried(n - len(body), body)
    r = _ref(w, brem)
    assert r["type"][0] == T_BLOB | F_CONT | (F_PARTIAL if brem > n else 0) and r["payload_off"][0] == 0
    cap = len(r["type"]) + 1
    got = _decode(ctx, kind, w, brem, cap)
    m, host = _check(got, w, brem, cap, (kind, case))
    _check_guard(host, m, (kind, case))
    assert (int(host["type"][0]), int(host["payload_off"][0]), int(host["payload_len"][0])) == \
        (T_BLOB | F_CONT | (F_PARTIAL if brem > n else 0), 0, brem)
    carry = got[6]
    if brem >= n:
        assert (got[2], carry.blob_remaining, carry.consumed, carry.tail_kind) == \
            (1, brem - n, n, TAIL_BLOB if brem > n else TAIL_NONE)
    else:
        assert got[2] == 1 + _ref(body, 0)["nframes"] and int(host["payload_off"][1]) == brem + 2


@pytest.mark.parametrize("brem", [0, 4099])
def test_malformed_change_is_kept(ctx, brem):
    """A Change without a required field in the middle: its row stays in the table (DRP_F_BAD |
    DRP_F_MISSING), err_code and err_frame are the oracle's (err_frame counts the carried blob's
    row), and nothing behind it is delivered."""
    from _gpu import drp_amd
    w = _carried(brem, BAD)
    r = _ref(w, brem)
    nf0 = 1 if brem else 0
    assert (r["nframes"], r["err_code"], r["err_frame"], len(r["type"])) == (nf0 + 20, M.ERR_REQUIRED, nf0 + 20, nf0 + 21)
    cap = nf0 + 61 + 2  # the whole chain and two rows to spare
    got = _decode(ctx, "device", w, brem, cap)
    assert got[0] == drp_amd.DRP_OK
    m, host = _check(got, w, brem, cap, ("malformed", brem))
    assert m == nf0 + 21 and int(host["flags"][m - 1]) & (M.F_BAD | M.F_MISSING) == M.F_BAD | M.F_MISSING
    # Differs from "nothing at or past min(cap, rows)" when rows counts the kept rows only: the
    # chain's 40 frames behind the malformed one are not delivered, but the kernels give every frame
    # of a chain a row (tests/test_gpu_change_matrix.py sizes its columns for that), and this path
    # decodes straight into the caller's columns, so rows [m, nf0 + 61) are written in every column.
    # Pinned as it is: those rows hold the frames' types, and nothing is written past the chain.
    assert (host["type"][m:nf0 + 61] == T_CHANGE).all()
    _check_guard(host, nf0 + 61, ("malformed", brem))


@pytest.mark.parametrize("brem,cap,ok", [(0, 299, False), (0, 300, True), (4099, 300, False), (4099, 301, True),
                                          (4099, 0, False), (5000 + len(C2), 0, False)])
def test_capacity(ctx, brem, cap, ok):
    """cap one short of the chain and cap == 0 with a carried blob: DRP_E_CAPACITY; cap exact:
    DRP_OK. A short capacity still reports the chain's counts and carry, the rows below cap are the
    oracle's, and no row at or past cap is written."""
    from _gpu import drp_amd
    w = _carried(min(brem, 5000), C2)
    got = _decode(ctx, "device", w, brem, cap)
    assert got[0] == (drp_amd.DRP_OK if ok else drp_amd.DRP_E_CAPACITY), got[0]
    if cap == 0:  # refused before anything is decoded or written
        _check_guard(got[1], 0, ("capacity", brem, cap))
        return
    m, host = _check(got, w, brem, cap, ("capacity", brem, cap))
    assert m == cap
    _check_guard(host, m, ("capacity", brem, cap))


@pytest.mark.parametrize("name,brem", [("c3", 0), ("c2", 4099), ("bad", 0)])
def test_device_key_hash_column(ctx, name, brem):
    """A non-null device key_hash column: the rows that are Changes get what
    decode_batch(key_hash=True) into host columns gives (the hash, and the key's class in the
    flags; 0 for the malformed Change), every other row of the column is left alone."""
    w = _carried(brem, {"c2": C2, "c3": C3, "bad": BAD}[name])
    r = _ref(w, brem)
    cap = len(r["type"]) + (40 if name == "bad" else 0) + 1
    key_ref = ctx.decode_batch(w, blob_remaining=brem, cap=cap, key_hash=True)
    ch = (r["type"] & 0x3F) == T_CHANGE
    good = ch & ((r["flags"] & M.F_BAD) == 0)
    assert good.sum() >= 20 and (key_ref["key_hash"][good] != 0).all() and (key_ref["flags"][good] & KEY_CLASS).all()
    got = _decode(ctx, "device", w, brem, cap, key_hash=True)
    m, host = _check(got, w, brem, cap, ("key_hash", name), key_ref=key_ref)
    if name == "bad":
        assert int(host["key_hash"][m - 1]) == 0 == int(key_ref["key_hash"][m - 1])
    _check_guard(host, m + (40 if name == "bad" else 0), ("key_hash", name))
