"""Relay measurement ("Relay"): drp_select_device against the column
probe, and the host relay through drp_relay_staged against the host round trip it replaces.

  device leg  --frames C2 frames resident in HBM and decoded; filter change <= 50 (half the
              rows); drp_select_device timed with HIP events on the ctx's stream; model bytes
              (58 B read per row, 61 B written per selected row) over the time; with --probe, the
              cols_rd figure of scripts/probe_bw.hip from a child process run just before.
  host leg    a --host-mib MiB host batch of the same stream, two paths on the same input,
              alternating, median of --runs runs each:
              (a) drp_decode_stage + drp_decode_fetch + numpy mask + drp_encode_batch
              (b) drp_decode_stage + drp_relay_staged
              and a check that both produce the same bytes.

Prints one JSON line (and writes it to --out). Needs an MI355X: there is no CPU path.

  hipcc -O3 --offload-arch=gfx950 scripts/probe_bw.hip -o exp/probe_bw
  python scripts/bench_relay.py --probe exp/probe_bw --out profiles/relay/relay_bench.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "dat-replication-protocol_amd", "python"))

READ_B, WRITE_B = 58, 61  # model bytes per row read / per selected row written (no sel_idx)
SRC_KEYS = ["key_off", "key_len", "subset_off", "subset_len", "value_off", "value_len", "change", "from", "to",
            "flags"]


def run_probe(path):
    """cols_rd (and the rest) of scripts/probe_bw.hip, TB/s per line."""
    out = subprocess.run([path], capture_output=True, text=True, timeout=300, check=True).stdout
    res = {}
    for line in out.splitlines():
        f = line.split()
        if len(f) >= 5 and f[2] == "ms" and f[4] == "TB/s":
            res[f[0]] = {"ms": float(f[1]), "TBps": float(f[3])}
    return res


def device_leg(ctx, drp_amd, torch, S, frames, iters):
    dev = torch.device("cuda", 0)
    wire = S.c2_stream(frames, seed=1)
    wire_t = torch.from_numpy(wire).to(dev)
    n = frames
    cap = n + 64
    cols = {"payload_off": torch.zeros(cap, dtype=torch.int64, device=dev),
            "payload_len": torch.zeros(cap, dtype=torch.int32, device=dev),
            "type": torch.zeros(cap, dtype=torch.uint8, device=dev),
            "flags": torch.zeros(cap, dtype=torch.uint8, device=dev)}
    for k in drp_amd.COLS32:
        cols[k] = torch.zeros(cap, dtype=torch.int32, device=dev)
    for k in drp_amd.COLS64:
        cols[k] = torch.zeros(cap, dtype=torch.int64, device=dev)
    so_t = torch.tensor([0, wire_t.numel()], dtype=torch.int64, device=dev)
    en_t = torch.zeros(1, dtype=torch.int64, device=dev)
    res_t = torch.zeros(C.sizeof(drp_amd.StreamResult), dtype=torch.uint8, device=dev)
    ctx.decode_device(wire_t, so_t, en_t, cols, cap, res_t)
    r = drp_amd.StreamResult.from_buffer_copy(res_t.cpu().numpy().tobytes())
    assert r.frames == n and r.err_code == 0, (r.frames, r.err_code)
    rows = {k: torch.zeros(n, dtype=(torch.int32 if k.endswith("_len") else torch.uint8 if k == "flags"
                                      else torch.int64), device=dev) for k in SRC_KEYS}
    nsel_t = torch.zeros(1, dtype=torch.int64, device=dev)
    flt = drp_amd.make_filter(change_range=(0, 50))
    ext = ctx._ext(dev)
    times = []
    for it in range(iters + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(ext)
        ctx.select_device(wire_t, cols, n, flt, rows, None, nsel_t)
        e1.record(ext)
        e1.synchronize()
        if it >= 3:  # (three warm-up launches)
            times.append(e0.elapsed_time(e1))
    nsel = int(nsel_t.cpu()[0])
    # the selection is the oracle-free closed form of the C2 stream: change = i % 100 + 1
    assert nsel == (n // 100) * 50 + min(n % 100, 50), nsel
    ch = rows["change"][:nsel].cpu().numpy()
    assert ch.max() <= 50 and ch.min() >= 1
    model = n * READ_B + nsel * WRITE_B
    ms = statistics.median(times)
    return {"frames": n, "selected": nsel, "model_bytes": model, "ms_median": ms, "ms_min": min(times),
            "ms_max": max(times), "iters": iters, "model_TBps": model / ms / 1e9}


def host_leg(ctx, drp_amd, S, mib, runs):
    L = ctx.L
    nbytes = mib << 20
    wire = S.c2_stream(nbytes // 86 + 1, seed=1)[:nbytes].copy()
    cap_rows = nbytes // 86 + 8
    host = drp_amd.alloc_host_outputs(cap_rows)
    fr, co = drp_amd._structs(host, drp_amd._p)
    out_a, out_b = np.zeros(nbytes, np.uint8), np.zeros(nbytes, np.uint8)
    flt = drp_amd.make_filter(change_range=(0, 50))
    U64, U32 = C.c_uint64, C.c_uint32

    def stage():
        carry = drp_amd.Carry(0, 0, 0, 0, 0)
        nf, ef, ec, ed = U64(), U64(), U32(), U32()
        rc = L.drp_decode_stage(ctx.h, drp_amd._p(wire), nbytes, C.byref(carry), C.byref(nf), C.byref(ef),
                                C.byref(ec), C.byref(ed))
        assert rc == 0 and ec.value == 0, (rc, ec.value)
        return int(nf.value)

    def path_a():
        n = stage()
        assert L.drp_decode_fetch(ctx.h, C.byref(fr), C.byref(co), 0, n) == 0
        keep = np.flatnonzero(((host["type"][:n] & 0x3F) == 1) & ((host["flags"][:n] & 4) == 0) &
                              (host["change"][:n] <= 50))
        po = host["payload_off"][keep]
        cols = {}
        for k in ["key", "subset", "value"]:
            cols[k + "_off"] = po + host[k + "_off"][keep]
            cols[k + "_len"] = host[k + "_len"][keep]
        for k in ["change", "from", "to"]:
            cols[k] = host[k][keep]
        cols["flags"] = host["flags"][keep] & 3
        src = drp_amd.ChangeSrc(*[drp_amd._p(np.ascontiguousarray(cols[k])) for k in SRC_KEYS])
        written = U64()
        rc = L.drp_encode_batch(ctx.h, C.byref(src), drp_amd._p(wire), nbytes, len(keep), drp_amd._p(out_a), nbytes,
                                C.byref(written))
        assert rc == 0, rc
        return int(written.value), len(keep)

    def path_b():
        stage()
        written, nsel = U64(), U64()
        rc = L.drp_relay_staged(ctx.h, C.byref(flt), drp_amd._p(out_b), nbytes, C.byref(written), C.byref(nsel))
        assert rc == 0, rc
        return int(written.value), int(nsel.value)

    for _ in range(2):  # warm-up: both paths, both arenas grown
        ra, rb = path_a(), path_b()
    same = ra == rb and out_a[:ra[0]].tobytes() == out_b[:rb[0]].tobytes()
    assert same, (ra, rb)
    ta, tb = [], []
    for _ in range(runs):  # alternating
        t0 = time.perf_counter()
        path_a()
        t1 = time.perf_counter()
        path_b()
        t2 = time.perf_counter()
        ta.append((t1 - t0) * 1e3)
        tb.append((t2 - t1) * 1e3)
    ma, mb = statistics.median(ta), statistics.median(tb)
    return {"batch_bytes": nbytes, "selected": ra[1], "out_bytes": ra[0], "runs": runs,
            "a_stage_fetch_mask_encode_ms": {"median": ma, "min": min(ta), "max": max(ta)},
            "b_stage_relay_ms": {"median": mb, "min": min(tb), "max": max(tb)}, "a_over_b": ma / mb,
            "same_bytes": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20_000_000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-mib", type=int, default=64)
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--probe", default=None, help="a built scripts/probe_bw.hip")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"bench": "relay"}
    if a.probe:
        res["probe_bw"] = run_probe(a.probe)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_relay.py needs an MI355X")
    torch.cuda.init()
    import _streams as S
    import drp_amd
    with drp_amd.Ctx(0) as ctx:
        ctx.set_blob_skip(drp_amd.BLOB_SKIP_OFF)
        res["device"] = device_leg(ctx, drp_amd, torch, S, a.frames, a.iters)
        if a.probe and "cols_rd" in res["probe_bw"]:
            res["device"]["over_cols_rd"] = res["device"]["model_TBps"] / res["probe_bw"]["cols_rd"]["TBps"]
        res["host"] = host_leg(ctx, drp_amd, S, a.host_mib, a.runs)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
