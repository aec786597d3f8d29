"""bench.py --dump-outputs (CPU): the files dump_outputs writes for a frame table larger than its
row sample: float32 / float64 only, the same seeded rows on every call, Change columns zeroed on
blob rows, and under 64 MB in all at the largest sample."""
import os

import numpy as np
import torch


def _table(n):
    import bench
    t = {"payload_off": torch.arange(n, dtype=torch.int64) * 86 + 2,
         "payload_len": torch.full((n,), 84, dtype=torch.int32),
         "type": torch.ones(n, dtype=torch.uint8), "flags": torch.full((n,), 2, dtype=torch.uint8)}
    t["type"][::7] = 2  # blobs: their Change columns hold whatever the buffer held
    for k in bench.drp_amd.COLS32:
        t[k] = torch.full((n + 64,), 9, dtype=torch.int32)  # (allocated with slack past n, as bench.py's)
    for k in bench.drp_amd.COLS64:
        t[k] = torch.arange(n + 64, dtype=torch.int64) + (1 << 33)
    return t


def test_dump_outputs_sample(tmp_path):
    import bench
    n = bench.DUMP_ROWS * 2 + 5
    t = _table(n)
    wire = np.arange(bench.DUMP_ELEMS + 3, dtype=np.int64).astype(np.uint8)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    for d in (a, b):
        bench.dump_outputs(d, t, n, [[n, 0, 0]], wire=wire, frame_off=torch.arange(100, dtype=torch.int64))
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    assert set(names) == {k + ".npy" for k in list(t) + ["rows", "result", "wire", "wire_index", "frame_off",
                                                         "frame_off_index"]}
    got = {f[:-4]: np.load(os.path.join(a, f)) for f in names}
    for f in names:
        assert got[f[:-4]].dtype in (np.float32, np.float64), f
        np.testing.assert_array_equal(got[f[:-4]], np.load(os.path.join(b, f)), err_msg=f)
    rows = got["rows"].astype(np.int64)
    assert 0 < rows.size <= bench.DUMP_ROWS and rows.max() < n and (np.diff(rows) > 0).all()
    np.testing.assert_array_equal(got["payload_off"], rows * 86 + 2)
    blob = rows % 7 == 0
    np.testing.assert_array_equal(got["type"], np.where(blob, 2, 1))
    np.testing.assert_array_equal(got["change"], np.where(blob, 0, rows + (1 << 33)))
    np.testing.assert_array_equal(got["key_len"], np.where(blob, 0, 9))
    np.testing.assert_array_equal(got["payload_len"], np.full(rows.size, 84))
    wi = got["wire_index"].astype(np.int64)
    assert wi.size <= bench.DUMP_ELEMS
    np.testing.assert_array_equal(got["wire"], wire[wi])
    np.testing.assert_array_equal(got["frame_off"], np.arange(100))
    # the largest dump: every table column and two further arrays at their full samples, with indices
    worst = (len(t) + 1) * bench.DUMP_ROWS * 8 + 2 * bench.DUMP_ELEMS * 16
    assert worst <= 64 * 10 ** 6
