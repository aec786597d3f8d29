"""Helpers of the tail tests (test_gpu_tail_chain.py, test_gpu_dual_scan.py): a context with
claims_fast's records on or off, and a device decode of cut streams checked against per-stream
oracle decodes."""
import ctypes as C
import os

import numpy as np

import _oracle as O


def tail_ctx(rec, **env):
    from _gpu import drp_amd
    env = {"DRP_CREC": str(rec), **env}
    keep = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        c = drp_amd.Ctx(0)
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    c.set_blob_skip(0)
    return c


def cut_entries(wire, cuts):
    """Per stream [cuts[s], cuts[s + 1]): the offset of the first frame that starts in it."""
    whole = O.decode_batch(wire)
    ends = whole["payload_off"].astype(np.int64) + whole["payload_len"].astype(np.int64)
    starts = np.concatenate([[0], ends[:-1]])
    entry = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        j = int(np.searchsorted(starts, a, "left"))
        entry.append(min(int(starts[j]) if j < len(starts) else b, b) - a)
    return entry, len(starts)


def stream_refs(wire, cuts, entry):
    return [O.decode_batch(wire[a + e:b]) for a, b, e in zip(cuts[:-1], cuts[1:], entry)]


def device_decode_check(c, wire, cuts, entry, refs, nrows):
    """drp_decode_device of the streams `cuts` of `wire`: every stream's result (frame_begin,
    frames, changes, blobs, error, tail) and every row against the per-stream oracle decodes."""
    import sys
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    from _gpu import COL_KEYS, drp_amd
    dev = torch.device("cuda", 0)
    ns = len(cuts) - 1
    cap = nrows + 64
    outs = bench.alloc_outputs(cap, dev)
    res = torch.zeros(ns * C.sizeof(drp_amd.StreamResult), dtype=torch.uint8, device=dev)
    w = torch.from_numpy(np.frombuffer(wire, np.uint8).copy()).to(dev)
    so = torch.tensor(cuts, dtype=torch.int64, device=dev)
    en = torch.tensor(entry, dtype=torch.int64, device=dev)
    c.decode_device(w, so, en, outs, cap, res)
    torch.cuda.synchronize()
    assert c.timing().strict_reruns == 0
    rs = np.frombuffer(res.cpu().numpy().tobytes(), np.uint8).reshape(ns, -1)
    host = {k: v.cpu().numpy() for k, v in outs.items()}
    row = 0
    for s in range(ns):
        ref = refs[s]
        r = drp_amd.StreamResult.from_buffer_copy(rs[s].tobytes())
        n = ref["nframes"]
        ch = (ref["type"][:n] & 0x3F) == 1
        got = (r.frame_begin, r.frames, r.changes, r.blobs, r.err_code, r.tail_kind)
        want = (row, n, int(ch.sum()), n - int(ch.sum()), ref["err_code"], ref["tail"])
        assert got == want, (s, got, want)
        sl = slice(row, row + n)
        np.testing.assert_array_equal(host["payload_off"][sl] - cuts[s] - entry[s],
                                      ref["payload_off"][:n].astype(np.int64), err_msg=f"stream {s}")
        np.testing.assert_array_equal(host["payload_len"][sl].astype(np.uint32), ref["payload_len"][:n],
                                      err_msg=f"stream {s}")
        np.testing.assert_array_equal(host["type"][sl], ref["type"][:n], err_msg=f"stream {s}")
        for k in COL_KEYS:
            np.testing.assert_array_equal(host[k][sl][ch].astype(ref[k].dtype), ref[k][:n][ch],
                                          err_msg=f"stream {s}:{k}")
        row += n
