"""GPU: the edges of the workgroup scans that no other test reaches.

- drp_index_scan (index_scan_kernel: one workgroup, 1024 values per round, a running carry) with
  more streams than one round takes: the wave edge, the round edge, the second and third round,
  and prefixes that pass 2^32 inside a round and across the carry.
- drp_fanout_latest_staged over 64 * 1024 + 1 rows: flat_scan_kernel gives each of its 1024
  threads a run of ceil(words / 1024) ballot words, and 1025 words is the first count at which a
  run holds more than one."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_fanout_latest import _fl, _pool_rows, _wire, ctx  # noqa: F401 (ctx: a fixture)

pytestmark = pytest.mark.gpu

GUARD = 0x5555555555555555
COUNTS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049, 3072]


def _frames(count, family, seed):
    """uint64 frame counts: below 2^20, or near 2^40 (two of them already pass 2^32: the prefix
    leaves 32 bits within the first wave, and the carry does at every round)."""
    rng = np.random.default_rng(seed)
    small = rng.integers(0, 1 << 20, count, dtype=np.uint64)
    return small if family == "small" else small + np.uint64(1 << 40)


@pytest.mark.parametrize("family", ["small", "near_2_40"])
@pytest.mark.parametrize("count", COUNTS)
def test_index_scan_past_one_round(ctx, count, family):  # noqa: F811
    """base[i] = the sum of frames[0, i) in uint64 for every count; the other three words of a
    record are noise; with count = 0 nothing is written."""
    import torch
    import drp_dist
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1000 + count)
    table = rng.integers(0, 1 << 63, (count, 4), dtype=np.uint64)
    table[:, 0] = _frames(count, family, seed=count)
    want = np.cumsum(table[:, 0], dtype=np.uint64) - table[:, 0]
    if count:
        assert int(want[-1]) + int(table[-1, 0]) == sum(int(x) for x in table[:, 0])  # (no wrap in the host's sum)
    if family == "near_2_40" and count > 1024:
        assert int(want[2]) >= 1 << 32 and int(want[1024]) >= 1 << 50
    table_t = torch.from_numpy(table.view(np.int64).copy()).to(dev)
    if count == 0:
        base_t = torch.full((1,), GUARD, dtype=torch.int64, device=dev)
        ctx.order_after_torch(base_t)
        assert ctx.L.drp_index_scan(ctx.h, C.c_void_p(table_t.data_ptr()), 0, C.c_void_p(base_t.data_ptr())) == 0
        assert ctx.L.drp_synchronize(ctx.h) == 0
        assert int(base_t.cpu()[0]) == GUARD
        assert drp_dist.global_index_device(ctx, table_t).shape == (0,)
        return
    base = drp_dist.global_index_device(ctx, table_t)
    np.testing.assert_array_equal(base.cpu().numpy().view(np.uint64), want)
    np.testing.assert_array_equal(table_t.cpu().numpy().view(np.uint64), table)  # (the table is read only)


def test_fanout_latest_two_words_per_thread(ctx):  # noqa: F811
    """65 537 rows are 1025 ballot words, two per thread of flat_scan_kernel: the smallest count
    whose run loop takes a second trip. The rows and filters of test_row_counts."""
    n = 64 * 1024 + 1
    rows = _pool_rows(n, n // 4, 5, seed=n, subsets=(None, None, b"s"))
    specs = [{}, {"change_range": (1, 3)}, {"subset": b"s"}]
    outs, want = _fl(ctx, _wire(rows), specs)
    assert all(0 < len(w[1]) < n for w in want)
    assert len({(k, sub) for k, sub, _ in rows}) < n  # (keys repeat)
