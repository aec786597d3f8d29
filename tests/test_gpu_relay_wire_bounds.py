"""The relay's wire bounds rule (wire_has / wire_eq of drp_select.h): a byte range outside
[0, nbytes) is never read and never matches. One stream of 130 Changes is decoded on the device,
then select, fan-out and latest-per-key get a wire cut short (the tensor's first `cut` bytes; the
memory behind it is still the whole tensor) with the columns of the whole stream. The expected
rows come from the oracle's columns: a byte condition holds only where its range ends at or before
the cut, a condition that reads no bytes does not notice the cut."""
import ctypes as C

import numpy as np
import pytest

import _oracle as O
import _streams as S
from _relay import SRC_KEYS, make_filter as _filter, rows as _rows

pytestmark = pytest.mark.gpu

N = 130  # three ballot words: the cuts fall inside the second
SPECS = [{"key_prefix": b"key"}, {"subset": b"ab"}, {"change_range": (1, 3)}]


@pytest.fixture(scope="module")
def ctx():
    from _gpu import drp_amd
    c = drp_amd.Ctx(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def decoded(ctx):
    """The wire and its device-decoded columns (shared, read only), and the oracle's columns."""
    import torch
    from _gpu import drp_amd
    dev = torch.device("cuda", 0)
    wire = b"".join(S.frame(S.change_payload(b"key%04d" % i, i % 7 + 1, 1, 2, value=b"v",
                                             subset=b"ab" if i % 2 else None)) for i in range(N))
    ref = O.decode_batch(wire)
    assert ref["nframes"] == N and ref["err_code"] == 0
    wire_t = torch.from_numpy(np.frombuffer(wire, np.uint8).copy()).to(dev)
    so_t = torch.tensor([0, len(wire)], dtype=torch.int64, device=dev)
    en_t = torch.zeros(1, dtype=torch.int64, device=dev)
    cap = N + 64
    cols = {"payload_off": torch.zeros(cap, dtype=torch.int64, device=dev),
            "payload_len": torch.zeros(cap, dtype=torch.int32, device=dev),
            "type": torch.zeros(cap, dtype=torch.uint8, device=dev),
            "flags": torch.zeros(cap, dtype=torch.uint8, device=dev)}
    for k in drp_amd.COLS32:
        cols[k] = torch.zeros(cap, dtype=torch.int32, device=dev)
    for k in drp_amd.COLS64:
        cols[k] = torch.zeros(cap, dtype=torch.int64, device=dev)
    rs = C.sizeof(drp_amd.StreamResult)
    res_t = torch.zeros(rs, dtype=torch.uint8, device=dev)
    ctx.decode_device(wire_t, so_t, en_t, cols, cap, res_t)
    res = drp_amd.StreamResult.from_buffer_copy(res_t.cpu().numpy().tobytes())
    assert res.frames == N
    for k in ["payload_off", "key_off", "subset_off", "key_len", "subset_len", "change", "flags"]:
        np.testing.assert_array_equal(cols[k][:N].cpu().numpy().astype(ref[k].dtype), ref[k][:N], err_msg=k)
    return wire_t, cols, ref


def _abs(ref, k):
    return ref["payload_off"][:N].astype(np.int64) + ref[k + "_off"][:N].astype(np.int64)


def _cuts(ref):
    at = int(_abs(ref, "key")[70])
    return {"inside": at + 2, "exact": at + 3, "zero": 0}


def _want(ref, spec, cut):
    """The rows `spec` keeps when the wire ends at `cut` (every row is a well-formed Change)."""
    i = np.arange(N)
    if "key_prefix" in spec:
        return np.flatnonzero(_abs(ref, "key") + len(spec["key_prefix"]) <= cut)
    if "subset" in spec:
        return np.flatnonzero((i % 2 == 1) & (_abs(ref, "subset") + len(spec["subset"]) <= cut))
    lo, hi = spec["change_range"]
    ch = ref["change"][:N].astype(np.int64)
    return np.flatnonzero((ch >= lo) & (ch <= hi))


def _out(room):
    import torch
    dev = torch.device("cuda", 0)
    rows = {k: torch.full((room,), 0x55, dtype=(torch.int32 if k.endswith("_len") else
                                               torch.uint8 if k == "flags" else torch.int64), device=dev)
            for k in SRC_KEYS}
    return rows, torch.full((room,), -1, dtype=torch.int64, device=dev)


def _run(ctx, decoded, cut, spec, fn):
    import torch
    wire_t, cols, _ = decoded
    rows, idx_t = _out(N)
    nsel_t = torch.full((1,), -1, dtype=torch.int64, device=wire_t.device)
    getattr(ctx, fn)(wire_t[:cut], cols, N, _filter(spec), rows, idx_t, nsel_t)
    torch.cuda.synchronize()
    nsel = int(nsel_t.cpu()[0])
    return {k: v.cpu().numpy()[:nsel] for k, v in rows.items()}, idx_t.cpu().numpy()[:nsel]


def _check(got, idx, ref, want_idx, what):
    np.testing.assert_array_equal(idx, want_idx, err_msg=str(what))
    want = _rows(ref, want_idx)
    for k in SRC_KEYS:
        np.testing.assert_array_equal(got[k].astype(want[k].dtype), want[k], err_msg=f"{what} {k}")


@pytest.mark.parametrize("name", ["inside", "exact", "zero"])
def test_wire_bounds(ctx, decoded, name):
    """inside: the cut leaves two bytes of row 70's key (the prefix "key" no longer fits: rows 0 .. 69
    match). exact: it ends right behind that prefix (row 70 matches too). zero: an empty wire (the
    byte conditions and latest keep nothing)."""
    import torch
    wire_t, cols, ref = decoded
    cut = _cuts(ref)[name]
    ak, asub = _abs(ref, "key"), _abs(ref, "subset")
    assert 0 <= cut < wire_t.numel()
    selected = []
    for spec in SPECS:
        got, idx = _run(ctx, decoded, cut, spec, "select_device")
        _check(got, idx, ref, _want(ref, spec, cut), ("select", name, spec))
        selected.append((got, idx))
    key_n = {"inside": 70, "exact": 71, "zero": 0}[name]
    assert len(selected[0][1]) == key_n and len(selected[1][1]) == (0 if name == "zero" else 35)
    assert len(selected[2][1]) == sum(1 for i in range(N) if i % 7 + 1 <= 3)  # (nothing is read: no cut)
    # fan-out: output f is the select's result for filter f, row for row
    total = sum(len(idx) for _, idx in selected)
    rows, idx_t = _out(total + 8)
    rb_t = torch.full((len(SPECS) + 1,), -1, dtype=torch.int64, device=wire_t.device)
    ctx.fanout_device(wire_t[:cut], cols, N, [_filter(s) for s in SPECS], rows, total, idx_t, rb_t)
    torch.cuda.synchronize()
    rb = rb_t.cpu().numpy()
    np.testing.assert_array_equal(rb, np.concatenate([[0], np.cumsum([len(idx) for _, idx in selected])]))
    fan_idx = idx_t.cpu().numpy()
    for f, (got, idx) in enumerate(selected):
        a, b = int(rb[f]), int(rb[f + 1])
        np.testing.assert_array_equal(fan_idx[a:b], idx, err_msg=f"fanout {f}")
        for k in SRC_KEYS:
            np.testing.assert_array_equal(rows[k].cpu().numpy()[a:b], got[k], err_msg=f"fanout {f} {k}")
    assert np.all(fan_idx[total:] == -1)
    # latest, no filter: a candidate's whole key, and its subset where it has one, lie within the
    # cut; the keys are distinct, so every candidate is its group's winner
    odd = np.arange(N) % 2 == 1
    cand = np.flatnonzero((ak + 7 <= cut) & (~odd | (asub + 2 <= cut)))
    got, idx = _run(ctx, decoded, cut, {}, "latest_device")
    _check(got, idx, ref, cand, ("latest", name))
    assert len(cand) == {"inside": 70, "exact": 70, "zero": 0}[name]
