"""The expected side every relay-family test shares (select, latest, fan-out, store, digest, order):
the select predicate and the winners per identity over the oracle's decode of a wire, the kept rows
as encoder rows, a decoded Change as a tuple, and the upload of a wire with its decoded columns.
Plain numpy and Python over _oracle's columns; nothing here runs on the device but device_cols."""
import collections

import numpy as np

import _oracle as O

SRC_KEYS = ["key_off", "key_len", "subset_off", "subset_len", "value_off", "value_len", "change", "from", "to",
            "flags"]
U64MAX = 2**64 - 1
Change = collections.namedtuple("Change", "has subset key change frm to hv value")


def bytes_at(wire, off, n):
    return bytes(wire[int(off):int(off) + int(n)])


def mask(wire, ref, n, spec):
    """The select predicate of `spec` (change_range / subset / subset_none / key_prefix; the
    conditions AND together) over the oracle's rows [0, n): numpy for the numbers and lengths, a byte
    compare per candidate."""
    ty, fl = ref["type"][:n], ref["flags"][:n]
    m = ((ty & 0x3F) == 1) & ((fl & 4) == 0)
    if spec.get("change_range") is not None:
        lo, hi = spec["change_range"]
        m &= (ref["change"][:n] >= np.uint64(lo)) & (ref["change"][:n] <= np.uint64(hi))
    if spec.get("subset_none"):
        m &= (fl & 1) == 0
    if spec.get("subset") is not None:
        want = spec["subset"]
        m &= ((fl & 1) != 0) & (ref["subset_len"][:n] == len(want))
        for i in np.flatnonzero(m):
            off = int(ref["payload_off"][i]) + int(ref["subset_off"][i])
            m[i] = bytes_at(wire, off, len(want)) == want
    if spec.get("key_prefix") is not None:
        want = spec["key_prefix"]
        m &= ref["key_len"][:n] >= len(want)
        for i in np.flatnonzero(m):
            off = int(ref["payload_off"][i]) + int(ref["key_off"][i])
            m[i] = bytes_at(wire, off, len(want)) == want
    return m


def rows(ref, idx, base=0):
    """Rows idx as encoder rows: offsets absolute (payload_off + column + base), flags masked to
    SUBSET | VALUE."""
    po = ref["payload_off"][idx].astype(np.uint64) + np.uint64(base)
    cols = {}
    for k in ["key", "subset", "value"]:
        cols[k + "_off"] = po + ref[k + "_off"][idx].astype(np.uint64)
        cols[k + "_len"] = ref[k + "_len"][idx].astype(np.uint32)
    for k in ["change", "from", "to"]:
        cols[k] = ref[k][idx].astype(np.uint64)
    cols["flags"] = (ref["flags"][idx] & 3).astype(np.uint8)
    return cols


def make_filter(spec):
    from _gpu import drp_amd
    return drp_amd.make_filter(**spec) if spec else None


def field_bytes(wire, cols, k, i):
    return bytes_at(wire, cols[k + "_off"][i], cols[k + "_len"][i])


def check_decoded(out, wire, cols):
    """The bytes `out` decode to the rows `cols` over `wire`: numbers, presence and key / subset /
    value bytes."""
    w, o = np.frombuffer(wire, np.uint8), np.frombuffer(out, np.uint8)
    d = O.decode_batch(out)
    n = len(cols["flags"])
    assert d["nframes"] == n and d["err_code"] == 0 and d["tail"] == 0, (d["nframes"], n, d["err_code"], d["tail"])
    assert np.all(d["type"][:n] == 1), "a frame of the output is no Change"
    for k in ["change", "from", "to"]:
        np.testing.assert_array_equal(d[k][:n], cols[k], err_msg=k)
    np.testing.assert_array_equal(d["flags"][:n] & 3, cols["flags"], err_msg="flags")
    dc = rows(d, np.arange(n))
    for i in range(n):
        for k, bit in [("key", 0), ("subset", 1), ("value", 2)]:
            if not bit or cols["flags"][i] & bit:
                got, want = field_bytes(o, dc, k, i), field_bytes(w, cols, k, i)
                assert got == want, f"row {i}, {k}: {got!r} != {want!r}"


def change_at(wire, ref, i):
    """Row i of the oracle's decode as a Change tuple."""
    po, fl = int(ref["payload_off"][i]), int(ref["flags"][i])
    f = lambda k: bytes_at(wire, po + int(ref[k + "_off"][i]), ref[k + "_len"][i])
    return Change(bool(fl & 1), f("subset") if fl & 1 else b"", f("key"), int(ref["change"][i]), int(ref["from"][i]),
                  int(ref["to"][i]), bool(fl & 2), f("value") if fl & 2 else b"")


def winners(wire, ref, cand):
    """Of the candidate rows `cand`, per identity (subset presence, subset bytes, key bytes) the row
    with the greatest (change, row). Returns (idx, best): the winners in increasing row order (numpy
    int64) and the dict from identity to its (change, row)."""
    best = {}
    for i in cand:
        i = int(i)
        po = int(ref["payload_off"][i])
        has = bool(ref["flags"][i] & 1)
        ident = (has, bytes_at(wire, po + int(ref["subset_off"][i]), ref["subset_len"][i]) if has else b"",
                 bytes_at(wire, po + int(ref["key_off"][i]), ref["key_len"][i]))
        cur = (int(ref["change"][i]), i)
        if ident not in best or cur > best[ident]:
            best[ident] = cur
    return np.array(sorted(i for _, i in best.values()), np.int64), best


def wire_winners(wire, spec=None, blob_remaining=0):
    """winners over the wire's delivered rows under `spec`, in the store tests' shape: (batch rows,
    Changes), in increasing row order."""
    ref = O.decode_batch(wire, blob_remaining=blob_remaining)
    idx, _ = winners(wire, ref, np.flatnonzero(mask(wire, ref, ref["nframes"], spec or {})))
    return [int(i) for i in idx], [change_at(wire, ref, int(i)) for i in idx]


def device_cols(ctx, wire, blob_remaining=0):
    """The wire on the device with its decoded columns (decode_staged's rows, uploaded): the
    arguments of merge_device / latest_device. The staged batch stays held."""
    import torch
    dev = torch.device("cuda", 0)
    g = ctx.decode_staged(wire, blob_remaining=blob_remaining)
    n = g["nframes"]
    cols = {}
    for k in ["payload_off", "payload_len", "type", "flags"] + O.COLS32 + O.COLS64:
        a = np.zeros(max(n, 1), g[k].dtype)
        a[:n] = g[k][:n]
        cols[k] = torch.from_numpy(signed(a)).to(dev)
    wire_t = torch.from_numpy(np.frombuffer(wire, np.uint8).copy()).to(dev)
    return wire_t, cols, n


# ---- encoder-row columns as numpy and as torch tensors (torch has no unsigned 32- and 64-bit dtypes) ----

def dtype(k):
    return np.uint32 if k.endswith("_len") else np.uint8 if k == "flags" else np.uint64


def signed(a):
    return a.view({1: np.uint8, 4: np.int32, 8: np.int64}[a.dtype.itemsize])


def up(a):
    import torch
    return torch.from_numpy(signed(np.ascontiguousarray(a)).copy()).to("cuda:0")


def down(t):
    a = t.cpu().numpy()
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
