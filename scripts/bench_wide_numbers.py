#!/usr/bin/env python3
"""C2-shaped decode with wide numbers: bench.c2_on_device's layout (10-digit key, 64 value bytes)
with change / from / to drawn U[2^28, 2^32) as 5-byte varints (98 B per frame), so every record
is a wide one (20 B stored; 24 B before the packed form). One JSON line: ms per decode (HIP
events around each step, median and all). Usage: python scripts/bench_wide_numbers.py
[--frames N] [--steps K] [--warmup W]; an A/B build by DRP_LIB=exp/<name>/libdrp.so."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from bench import drp_amd  # noqa: E402

FRAME = 98


def wide_on_device(nframes, seed, dev):
    a = torch.empty((nframes, FRAME), dtype=torch.uint8, device=dev)
    i = torch.arange(nframes, device=dev, dtype=torch.int64)
    a[:, 0], a[:, 1], a[:, 2], a[:, 3] = FRAME - 1, 1, 0x12, 10
    for k in range(10):
        a[:, 4 + k] = (48 + torch.div(i, 10 ** (9 - k), rounding_mode="floor") % 10).to(torch.uint8)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    nums = torch.randint(2 ** 28, 2 ** 32, (nframes, 3), generator=g, device=dev, dtype=torch.int64)
    for f in range(3):
        c = 14 + 6 * f
        a[:, c] = 0x18 + 8 * f
        for b in range(5):
            a[:, c + 1 + b] = (((nums[:, f] >> (7 * b)) & 0x7F) | (0x80 if b < 4 else 0)).to(torch.uint8)
    a[:, 32], a[:, 33] = 0x32, 64
    a[:, 34:] = torch.randint(0, 256, (nframes, 64), generator=g, device=dev, dtype=torch.uint8)
    return a.reshape(-1), nums


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = args.frames
    wire, nums = wide_on_device(n, 5, dev)
    so = torch.tensor([0, wire.numel()], dtype=torch.int64, device=dev)
    outs = bench.alloc_outputs(n + 64, dev)
    res = torch.zeros(C.sizeof(drp_amd.StreamResult), dtype=torch.uint8, device=dev)
    ctx = drp_amd.Ctx(0)
    ext = torch.cuda.ExternalStream(ctx.stream, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for s in range(args.warmup + args.steps):
        ev[0].record(ext)
        ctx.decode_device(wire, so, None, outs, n + 64, res)
        ev[1].record(ext)
        torch.cuda.synchronize(dev)
        if s >= args.warmup:
            ms.append(ev[0].elapsed_time(ev[1]))
    r = drp_amd.StreamResult.from_buffer_copy(res.cpu().numpy().tobytes()[:C.sizeof(drp_amd.StreamResult)])
    assert (r.frames, r.changes, r.err_code, r.consumed) == (n, n, 0, n * FRAME), (r.frames, r.err_code)
    for f, k in enumerate(["change", "from", "to"]):
        assert torch.equal(outs[k][:n], nums[:, f]), k
    assert bool((outs["value_off"][:n] == 32).all()) and bool((outs["value_len"][:n] == 64).all())
    t = ctx.timing()
    print(json.dumps({"workload": f"C2-shaped, 5-byte numbers: {n} frames x {FRAME} B", "lib": os.environ.get("DRP_LIB"),
                      "ms_per_step": statistics.median(ms), "ms": ms, "spec_repairs": t.spec_repairs,
                      "strict_reruns": t.strict_reruns}))
    ctx.close()


if __name__ == "__main__":
    main()
