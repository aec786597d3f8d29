#!/usr/bin/env python3
"""Benchmark: decoded Change frames/s + wire GB/s on MI355X (BASELINE.json metric).

Workload (BASELINE.json configs[1]): per GPU one 8.6 GB replication
stream of 100,000,000 Change frames of exactly 86 B (10-digit key, change=(i%100)+1,
from=i%128, to=(i+1)%128, 64 random value bytes), synthesised on the device (seeded) and
resident in HBM before timing. One step = one full decode of that stream by libdrp
(frame split + Change decode into SoA columns, decode.js:144-262 + messages/index.js:5)
plus, for N > 1, the RCCL all-gather of per-stream stats and the global index scan.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--frames F] [--dump-outputs DIR] [--full]
    torchrun --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 bench.py --gpus N

Prints ONE JSON line (rank 0). A plain run sets up, warms up (checking the decoded columns
against the generator), times the K steps and prints the line; `roofline` prices the decode
kernel from the HIP events libdrp records around it in those same steps. --dump-outputs DIR
also writes what the last timed step computed as DIR/<name>.npy (dump_outputs). --full adds
every other leg: the c4 / c5 / c3 sub-lines, `cpu_baseline*` (the C restatement of the
reference, oracle/, on a bounded sample on this host's cores), the H2D rate, the Node path,
C5's decode-after-C2 leg and C3's HBM-resident roofline leg.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "dat-replication-protocol_amd", "python"))
import drp_amd  # noqa: E402
import drp_dist  # noqa: E402

HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md)
# the speculative decode's kernels (drp_decode_spec.hip, drp_walk.hip) for batches of >= 32768 tiles
DECODE_PATH = ("speculative decode: walk_regions + walk_sync + walk_density, then claims_fast (dense) or the hop "
               "walkers (sparse) by a 16-byte density read-back + spec_claims + verify_lite + tile scans + emit")
FRAME = 86


def c2_on_device(nframes, seed, dev):
    """C2 stream generated on the GPU (same layout as tests/_streams.c2_stream)."""
    a = torch.empty((nframes, FRAME), dtype=torch.uint8, device=dev)
    i = torch.arange(nframes, device=dev, dtype=torch.int64)
    a[:, 0] = 85
    a[:, 1] = 1
    a[:, 2] = 0x12
    a[:, 3] = 10
    for k in range(10):
        a[:, 4 + k] = (48 + torch.div(i, 10 ** (9 - k), rounding_mode="floor") % 10).to(torch.uint8)
    a[:, 14] = 0x18
    a[:, 15] = ((i % 100) + 1).to(torch.uint8)
    a[:, 16] = 0x20
    a[:, 17] = (i % 128).to(torch.uint8)
    a[:, 18] = 0x28
    a[:, 19] = ((i + 1) % 128).to(torch.uint8)
    a[:, 20] = 0x32
    a[:, 21] = 64
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    a[:, 22:] = torch.randint(0, 256, (nframes, 64), generator=g, device=dev, dtype=torch.uint8)
    del i
    return a.reshape(-1)


def alloc_outputs(cap, dev):
    o = {"payload_off": torch.empty(cap, dtype=torch.int64, device=dev),
         "payload_len": torch.empty(cap, dtype=torch.int32, device=dev),
         "type": torch.empty(cap, dtype=torch.uint8, device=dev),
         "flags": torch.empty(cap, dtype=torch.uint8, device=dev)}
    for k in drp_amd.COLS32:
        o[k] = torch.empty(cap, dtype=torch.int32, device=dev)
    for k in drp_amd.COLS64:
        o[k] = torch.empty(cap, dtype=torch.int64, device=dev)
    return o


DUMP_ROWS = 1 << 18       # rows of the frame table --dump-outputs keeps
DUMP_ELEMS = 1 << 20      # elements it keeps of any other output array (under 64 MB in all)
CHANGE_COLS = drp_amd.COLS32 + drp_amd.COLS64 + ["flags"]


def _dump_pick(n, limit, seed):
    """Every index below n, or a fixed sorted sample of at most `limit` of them (seeded: the same
    rows in every run with the same arguments)."""
    if n <= limit:
        return np.arange(n, dtype=np.int64)
    return np.unique(np.random.default_rng(seed).integers(0, n, size=limit, dtype=np.int64))


def _dump_take(v, idx):
    """v[idx] on the host: float32 for byte arrays, float64 otherwise (exact: every value the
    benchmark's workloads decode is an integer below 2^53)."""
    if isinstance(v, torch.Tensor):
        v = v[torch.from_numpy(idx).to(v.device)].cpu().numpy()
    else:
        v = np.asarray(v)[idx]
    return v.astype(np.float32 if v.dtype.itemsize == 1 else np.float64)


def dump_outputs(path, table, n, result, **arrays):
    """--dump-outputs: what the last timed step left in the caller's buffers, as <path>/<name>.npy.
    `table`: the frame table's columns (torch or numpy, n rows), one file per column. Past
    DUMP_ROWS rows a seeded sample of rows is kept and rows.npy holds their indices. The Change
    columns are written as 0 on rows that are not Changes (the decoder does not write them there).
    `result`: the per-stream results (a 2-D array, result.npy). `arrays`: further 1-D outputs,
    each whole or as a seeded sample of DUMP_ELEMS elements with its indices in <name>_index.npy."""
    os.makedirs(path, exist_ok=True)
    idx = _dump_pick(n, DUMP_ROWS, seed=20)
    np.save(os.path.join(path, "rows.npy"), idx.astype(np.float64))
    got = {k: _dump_take(v, idx) for k, v in table.items()}
    change = (got["type"].astype(np.uint8) & 0x3F) == drp_amd.TYPE_CHANGE
    for k, v in got.items():
        np.save(os.path.join(path, k + ".npy"), np.where(change, v, 0).astype(v.dtype) if k in CHANGE_COLS else v)
    np.save(os.path.join(path, "result.npy"), np.asarray(result, dtype=np.float64))
    for k, v in arrays.items():
        idx = _dump_pick(len(v), DUMP_ELEMS, seed=21)
        np.save(os.path.join(path, k + "_index.npy"), idx.astype(np.float64))
        np.save(os.path.join(path, k + ".npy"), _dump_take(v, idx))


def stream_results(res):
    """The StreamResult records of a device decode as a float64 array, one row per stream
    (every field but the reserved one, in declaration order)."""
    r = np.frombuffer(res.cpu().numpy().tobytes(), dtype=np.dtype(drp_amd.StreamResult))
    return np.stack([r[f].astype(np.float64) for f, _ in drp_amd.StreamResult._fields_ if f != "reserved"], axis=1)


def verify_c2(o, res, nframes, dev):
    """Size-independent properties of the full-size decode (bit-exact vs the generator)."""
    r = drp_amd.StreamResult.from_buffer_copy(res.cpu().numpy().tobytes()[:C.sizeof(drp_amd.StreamResult)])
    o = {k: v[:nframes] for k, v in o.items()}  # columns are allocated with slack past nframes
    assert (r.frames, r.changes, r.blobs, r.err_code, r.tail_kind, r.consumed) == \
        (nframes, nframes, 0, 0, 0, nframes * FRAME), (r.frames, r.err_code, r.tail_kind, r.consumed)
    i = torch.arange(nframes, device=dev, dtype=torch.int64)
    checks = {
        "payload_off": torch.equal(o["payload_off"], i * FRAME + 2),
        "payload_len": bool((o["payload_len"] == 84).all()), "type": bool((o["type"] == 1).all()),
        "key_off": bool((o["key_off"] == 2).all()), "key_len": bool((o["key_len"] == 10).all()),
        "value_off": bool((o["value_off"] == 20).all()), "value_len": bool((o["value_len"] == 64).all()),
        "subset_len": bool((o["subset_len"] == 0).all()), "flags": bool((o["flags"] == 2).all()),
        "change": torch.equal(o["change"], (i % 100) + 1), "from": torch.equal(o["from"], i % 128),
        "to": torch.equal(o["to"], (i + 1) % 128),
    }
    bad = [k for k, v in checks.items() if not v]
    assert not bad, f"decoded columns differ from the generator: {bad}"


def host_cores():
    """Cores this process may use: the box's CPU share (OMP_NUM_THREADS is set to it there),
    never more than the affinity mask."""
    avail = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    want = int(os.environ.get("OMP_NUM_THREADS") or avail)
    return max(1, min(want, avail))


def calibration(port_frames_per_s):
    """BASELINE.md "Calibration": the reference JS (decode.js in place) over the C restatement,
    both timed on one core of the build container (profiles/calibration_ref_js.json, from
    scripts/calibrate_reference.py); applied to the port's rate on this host it estimates what
    the reference itself would decode here (it cannot run on the GPU box)."""
    try:
        with open(os.path.join(ROOT, "profiles", "calibration_ref_js.json")) as f:
            c = json.load(f)
    except (OSError, ValueError):
        return None
    r = c["ratio_ref_js_over_port"]
    return {"ratio_ref_js_over_port": r, "reference_js_equiv_frames_per_s": port_frames_per_s * r,
            "measured": {"reference_js_frames_per_s": c["reference_js"]["frames_per_s"],
                         "port_frames_per_s": c["port_c"]["frames_per_s"], "where": "build container, 1 core",
                         "workload": c["workload"]}}


def _oracle_modules():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _oracle as O
    import _streams as S
    return O, S


def cpu_baseline(min_seconds=10.0, sample_frames=2_000_000):
    """The C restatement of decode.js (oracle/, 1 thread) over a C2 sample in 64 KiB writes."""
    O, S = _oracle_modules()
    wire = S.c2_stream(sample_frames, seed=7).tobytes()
    outs = O.alloc_outputs(sample_frames + 16)
    O.decode_batch(wire, chunk=65536, outs=outs)
    reps, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < min_seconds:
        r = O.decode_batch(wire, chunk=65536, outs=outs)
        assert r["nframes"] == sample_frames
        reps += 1
    dt = time.perf_counter() - t0
    v = reps * sample_frames / dt
    return {"value": v, "unit": "frames/s", "cores": 1, "kind": "port",
            "wire_GBps": reps * len(wire) / dt / 1e9,
            "sample": f"C2 sample of {sample_frames} frames ({len(wire)} B) decoded {reps}x in 64 KiB "
                      f"writes by oracle/drp_oracle.c (decode.js + protocol-buffers@2 restatement), "
                      f"{dt:.1f} s on 1 host core",
            "calibration": calibration(v)}


def cpu_baseline_streams(min_seconds=10.0, streams_per_core=2, seed=4):
    """C4 on every host core (BASELINE.md plan): one thread per core, each decoding its own
    independent C4 streams (U[8192,16384] C2 frames) with the C restatement in 64 KiB writes
    (ctypes releases the GIL, so the threads run in parallel)."""
    import threading
    O, S = _oracle_modules()
    cores = host_cores()
    rng = np.random.default_rng(seed)
    counts = rng.integers(8192, 16385, size=cores * streams_per_core)
    work = [[S.c2_stream(int(n), seed=seed * 1000 + k).tobytes()
             for k, n in enumerate(counts[c * streams_per_core:(c + 1) * streams_per_core])] for c in range(cores)]
    done = [0] * cores
    t_end = [0.0]

    def run(c):
        outs = O.alloc_outputs(16385 + 16)
        while time.perf_counter() < t_end[0]:
            for w in work[c]:
                r = O.decode_batch(w, chunk=65536, outs=outs)
                done[c] += r["nframes"]

    t0 = time.perf_counter()
    t_end[0] = t0 + min_seconds
    ts = [threading.Thread(target=run, args=(c,)) for c in range(cores)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    dt = time.perf_counter() - t0
    v = sum(done) / dt
    return {"value": v, "unit": "frames/s", "cores": cores, "kind": "port",
            "wire_GBps": v * FRAME / 1e9,
            "sample": f"C4 sample: {len(counts)} independent streams of U[8192,16384] C2 frames, "
                      f"{streams_per_core} per thread, {cores} threads, decoded repeatedly in 64 KiB writes "
                      f"by oracle/drp_oracle.c for {dt:.1f} s",
            "calibration": calibration(v / cores)}


def cpu_baseline_c5(min_seconds=10.0, rows_per_core=4000, seed=55):
    """C5 round trip on every host core: each thread encodes its own C5-shaped rows (4096 B
    values, key U[1,256], change/from/to U[0,2^32)) with the C restatement of encode.js +
    protocol-buffers@2 and decodes the wire back in 64 KiB writes."""
    import threading
    O, S = _oracle_modules()
    cores = host_cores()
    rng = np.random.default_rng(seed)
    jobs = []
    for c in range(cores):
        kl = rng.integers(1, 257, size=rows_per_core).astype(np.uint32)
        row = kl.astype(np.uint64) + C5_VALUE
        ko = np.cumsum(row) - row
        heap = rng.integers(0, 256, size=int(row.sum()), dtype=np.uint8).tobytes()
        nums = rng.integers(0, 1 << 32, size=(3, rows_per_core), dtype=np.uint64)
        cols = {"key_off": ko.astype(np.uint64), "key_len": kl, "subset_off": np.zeros(rows_per_core, np.uint64),
                "subset_len": np.zeros(rows_per_core, np.uint32), "value_off": (ko + kl).astype(np.uint64),
                "value_len": np.full(rows_per_core, C5_VALUE, np.uint32), "change": nums[0], "from": nums[1],
                "to": nums[2], "flags": np.full(rows_per_core, 2, np.uint8)}
        jobs.append((heap, cols))
    done = [0] * cores
    t_end = [0.0]

    def run(c):
        heap, cols = jobs[c]
        outs = O.alloc_outputs(rows_per_core + 16)
        while time.perf_counter() < t_end[0]:
            wire = O.encode_changes(heap, cols)
            r = O.decode_batch(wire, chunk=65536, outs=outs)
            assert r["nframes"] == rows_per_core
            done[c] += rows_per_core

    t0 = time.perf_counter()
    t_end[0] = t0 + min_seconds
    ts = [threading.Thread(target=run, args=(c,)) for c in range(cores)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    dt = time.perf_counter() - t0
    return {"value": sum(done) / dt, "unit": "frames/s", "cores": cores, "kind": "port",
            "sample": f"C5 sample: {rows_per_core} rows per thread, {cores} threads, encode -> decode "
                      f"(64 KiB writes) by oracle/drp_oracle.c repeatedly for {dt:.1f} s"}


def node_path(frames=4_000_000, reps=3):
    """The product path (north_star: Node host over the N-API addon) on a C2 sample: the
    package's Decoder fed 64 KiB writes (coalesced per event-loop turn, up to 64 MiB per GPU
    call) and 256 MiB writes (one GPU call each), with no-op change callbacks. Reported apart
    from the kernel number: it includes H2D, the D2H of the columns and the per-frame JS replay
    (building each {subset,key,change,from,to,value} object)."""
    import shutil
    import subprocess
    import tempfile
    node = shutil.which("node")
    if node is None:
        return {"skipped": "node not installed on this host"}
    _, S = _oracle_modules()
    wire = S.c2_stream(frames, seed=9).tobytes()
    out = {"workload": f"C2 sample, {frames} frames x 86 B, change callbacks acknowledged synchronously"}
    with tempfile.NamedTemporaryFile(suffix=".bin", delete=False) as f:
        f.write(wire)
        path = f.name
    try:
        for name, write, batch in [("writes_64KiB", 65536, 64 << 20), ("writes_256MiB", 256 << 20, 256 << 20)]:
            env = dict(os.environ, DRP_MAX_BATCH=str(batch))
            r = subprocess.run([node, os.path.join(ROOT, "scripts", "bench_node.js"), path, str(write), str(reps)],
                               env=env, capture_output=True, text=True, timeout=600)
            out[name] = json.loads(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 else \
                {"error": (r.stderr or r.stdout)[-400:]}
    finally:
        os.unlink(path)
    # the Encoder (encode.js over the addon): change() calls -> GPU encode per tick batch -> a
    # discarding sink; the reference's own encoder measured in the build container (BASELINE.md,
    # shim codec): 0.19 M frames/s for 1M x 64 B values, 0.14 M frames/s for 200k x 4 KB values
    for name, shape, rows, ref in [("encode_c1", "c1", 1_000_000, 0.19e6), ("encode_c5", "c5", 200_000, 0.14e6)]:
        r = subprocess.run([node, os.path.join(ROOT, "scripts", "bench_node_encode.js"), shape, str(rows), "3"],
                           capture_output=True, text=True, timeout=600)
        if r.returncode == 0:
            out[name] = json.loads(r.stdout.strip().splitlines()[-1])
            out[name]["reference_js_container_frames_per_s"] = ref
            out[name]["vs_reference_js_container"] = out[name]["frames_per_s"] / ref
        else:
            out[name] = {"error": (r.stderr or r.stdout)[-400:]}
    return out


def h2d_rate(dev, nbytes=1 << 30):
    """Pinned host -> HBM copy rate for one batch (reported separately, never `value`)."""
    h = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    d = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    d.copy_(h, non_blocking=True)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(3):
        d.copy_(h, non_blocking=True)
    torch.cuda.synchronize(dev)
    dt = (time.perf_counter() - t0) / 3
    del h, d
    return {"GBps": nbytes / dt / 1e9, "bytes": nbytes, "note": "pinned host -> HBM, 1 GiB batch"}


def c4_on_device(nstreams_total, rank, world, dev, seed=4):
    """C4: 8192 independent streams, stream s has U[8192,16384] C2-shaped frames
    (seeded, identical on every rank); this rank decodes the contiguous block drp_dist gives it."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(8192, 16385, size=nstreams_total, dtype=np.int64)
    lo, hi = drp_dist.shard_range(nstreams_total, world, rank)
    mine = counts[lo:hi]
    nframes = int(mine.sum())
    wire = c2_on_device(nframes, seed=seed * 1000 + rank, dev=dev)
    stream_off = torch.from_numpy(np.concatenate([[0], np.cumsum(mine)]) * FRAME).to(dev)
    return wire, stream_off, mine, (lo, hi)


def verify_c4(o, res, counts, base, lo, dev):
    """Size-independent properties: per-stream frame counts, clean ends, dense in-order
    frame table and the all-gathered global index."""
    rs = C.sizeof(drp_amd.StreamResult)
    raw = res.cpu().numpy().tobytes()
    begin = 0
    for s, n in enumerate(counts):
        r = drp_amd.StreamResult.from_buffer_copy(raw[s * rs:(s + 1) * rs])
        assert (r.frame_begin, r.frames, r.changes, r.err_code, r.tail_kind, r.consumed) == \
            (begin, n, n, 0, 0, n * FRAME), (s, r.frame_begin, r.frames, r.err_code)
        begin += int(n)
    nf = int(counts.sum())
    i = torch.arange(nf, device=dev, dtype=torch.int64)
    assert torch.equal(o["payload_off"][:nf], i * FRAME + 2), "payload offsets"
    assert bool((o["value_len"][:nf] == 64).all()) and bool((o["flags"][:nf] == 2).all())
    if base is not None:
        exp = torch.cumsum(torch.as_tensor(counts, device=dev), 0) - torch.as_tensor(counts, device=dev)
        assert torch.equal(base[lo:lo + len(counts)] - base[lo], exp), "global index"


C5_VALUE = 4096


def varint_len(x):
    """LEB128 length of non-negative int64 values below 2^35 (varint@3 encode)."""
    return 1 + (x >= 1 << 7).long() + (x >= 1 << 14).long() + (x >= 1 << 21).long() + (x >= 1 << 28).long()


def c5_on_device(n, seed, dev):
    """C5: n Changes with 4096 random value bytes, key length U[1,256] and
    change/from/to U[0,2^32), as encoder columns over one device heap (key then value per row).
    Returns the columns, the heap and the expected frame sizes (encode.js:102-137 layout)."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    key_len = torch.randint(1, 257, (n,), generator=g, device=dev, dtype=torch.int64)
    nums = torch.randint(0, 1 << 32, (3, n), generator=g, device=dev, dtype=torch.int64)
    row = key_len + C5_VALUE
    key_off = torch.cumsum(row, 0) - row
    heap = torch.randint(0, 256, (int(row.sum()),), generator=g, device=dev, dtype=torch.uint8)
    cols = {"key_off": key_off, "key_len": key_len.to(torch.int32),
            "subset_off": torch.zeros(n, dtype=torch.int64, device=dev),
            "subset_len": torch.zeros(n, dtype=torch.int32, device=dev),
            "value_off": key_off + key_len,
            "value_len": torch.full((n,), C5_VALUE, dtype=torch.int32, device=dev),
            "change": nums[0].contiguous(), "from": nums[1].contiguous(), "to": nums[2].contiguous(),
            "flags": torch.full((n,), 2, dtype=torch.uint8, device=dev)}
    payload = (1 + varint_len(key_len) + key_len) + (3 + varint_len(nums).sum(0)) + \
        (1 + varint_len(torch.full_like(key_len, C5_VALUE)) + C5_VALUE)
    frame = varint_len(payload + 1) + 1 + payload
    return cols, heap, frame


def verify_c5(cols, heap, wire, o, res, n, dev, samples=256):
    """Round-trip properties at full size: every decoded column equals the encoder's input and
    sampled key/value bytes in the wire equal the heap's (bit-exact)."""
    r = drp_amd.StreamResult.from_buffer_copy(res.cpu().numpy().tobytes()[:C.sizeof(drp_amd.StreamResult)])
    assert (r.frames, r.changes, r.err_code, r.tail_kind, r.consumed) == (n, n, 0, 0, wire.numel()), \
        (r.frames, r.err_code, r.tail_kind, r.consumed)
    o = {k: v[:n] for k, v in o.items()}
    for k in ["change", "from", "to"]:
        assert torch.equal(o[k], cols[k]), k
    for k in ["key_len", "value_len"]:
        assert torch.equal(o[k], cols[k]), k
    assert bool((o["flags"] == 2).all()) and bool((o["subset_len"] == 0).all()) and bool((o["type"] == 1).all())
    g = torch.Generator(device="cpu")
    g.manual_seed(5)
    for i in torch.randint(0, n, (samples,), generator=g).tolist():
        po = int(o["payload_off"][i])
        for off_w, off_h, ln in [(int(o["key_off"][i]), int(cols["key_off"][i]), int(cols["key_len"][i])),
                                 (int(o["value_off"][i]), int(cols["value_off"][i]), C5_VALUE)]:
            assert torch.equal(wire[po + off_w:po + off_w + ln], heap[off_h:off_h + ln]), i


def run_c5(args, dev, rank=0, world=1, steps=None, warmup=None, cpu=True, dump=None):
    """C5: batched encode -> decode round trip of 1M Changes with 4 KB values per step per GPU
    (BASELINE configs[4]: 8 x MI355X); each rank round-trips its own rows (weak scaling), then the
    32 B per-stream stats are all-gathered (drp_index_allgather over RCCL; gloo only to rehearse
    ranks on one GPU). value = Changes round-tripped per second, whole job. Returns rank 0's line.
    dump: rank 0 writes the last timed step's wire, frame offsets and decoded table there."""
    dist = world > 1
    steps = args.steps if steps is None else steps
    warmup = args.warmup if warmup is None else warmup
    n = args.c5_changes
    cols, heap, frame = c5_on_device(n, seed=55 + rank, dev=dev)
    W = int(frame.sum())
    out = torch.empty(W + 64, dtype=torch.uint8, device=dev)
    foff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    wire = out[:W]
    stream_off = torch.tensor([0, W], dtype=torch.int64, device=dev)
    cap = n + 64
    outs = alloc_outputs(cap, dev)
    res = torch.zeros(C.sizeof(drp_amd.StreamResult), dtype=torch.uint8, device=dev)
    ctx = drp_amd.Ctx(dev.index)
    ext = torch.cuda.ExternalStream(ctx.stream, device=dev)
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    enc_ms, dec_ms = [], []
    state = {"base": None}

    def step(timed):
        evs[0].record(ext)
        ctx.encode_device(cols, heap, n, foff, out, W + 64)
        evs[1].record(ext)
        ctx.decode_device(wire, stream_off, None, outs, cap, res)
        evs[2].record(ext)
        if dist:  # the only collective: one 32-byte stats record per rank's stream
            stats = drp_dist.local_stats_device(ctx, res, stream_off)
            if args.backend == "nccl":
                _, state["base"] = drp_dist.global_index_rccl(ctx, stats, world)
            else:
                state["base"] = drp_dist.global_index_device(ctx, drp_dist.gather_stats(stats, world))
        if timed:
            torch.cuda.synchronize(dev)
            enc_ms.append(evs[0].elapsed_time(evs[1]))
            dec_ms.append(evs[1].elapsed_time(evs[2]))

    for _ in range(max(1, warmup)):
        step(False)
    torch.cuda.synchronize(dev)
    assert int(foff[n]) == W, (int(foff[n]), W)
    assert torch.equal(foff[1:] - foff[:-1], frame), "frame sizes differ from the encode.js layout"
    verify_c5(cols, heap, wire, outs, res, n, dev)
    if dist:  # every rank's stream holds n frames: the global index of rank r's stream is r * n
        assert torch.equal(state["base"].cpu(), torch.arange(world, dtype=torch.int64) * n), state["base"]
        torch.distributed.barrier()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    with torch.cuda.stream(ext):  # (torch's stream is libdrp's: no cross-stream waits per call)
        for _ in range(steps):
            step(True)
    torch.cuda.synchronize(dev)
    if dist:
        torch.distributed.barrier()
    elapsed = time.perf_counter() - t0
    t = ctx.timing()
    if dist:
        cdev = dev if args.backend == "nccl" else torch.device("cpu")
        tt = torch.tensor([elapsed], dtype=torch.float64, device=cdev)
        torch.distributed.all_reduce(tt, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(tt.item())
    if dump and rank == 0:
        dump_outputs(dump, outs, n, stream_results(res), wire=wire, frame_off=foff)
    # the same context right after a dense C2 batch: the claims form is chosen per launch on the
    # device (walk_sync's density sample), not from the context's previous decode
    after_c2 = None
    if rank == 0 and args.full and not args.no_after_c2:
        nf2 = 10_000_000
        w2 = c2_on_device(nf2, seed=99, dev=dev)
        so2 = torch.tensor([0, w2.numel()], dtype=torch.int64, device=dev)
        o2 = alloc_outputs(nf2 + 64, dev)
        r2 = torch.zeros(C.sizeof(drp_amd.StreamResult), dtype=torch.uint8, device=dev)
        ms = []
        with torch.cuda.stream(ext):
            for _ in range(3):
                ctx.decode_device(w2, so2, None, o2, nf2 + 64, r2)
                evs[1].record(ext)
                ctx.decode_device(wire, stream_off, None, outs, cap, res)
                evs[2].record(ext)
                torch.cuda.synchronize(dev)
                ms.append(evs[1].elapsed_time(evs[2]))
        t2 = ctx.timing()
        verify_c5(cols, heap, wire, outs, res, n, dev)
        after_c2 = {"ms": float(np.median(ms)), "exact_fallbacks": t2.strict_reruns, "repair_passes": t2.spec_repairs,
                    "segmented_repairs": t2.seg_repairs, "note": "C5 decode right after a 10M-frame C2 decode on the "
                    "same context (median of 3)"}
        del w2, o2, r2
    H = int(heap.numel())
    e, d = float(np.mean(enc_ms)) / 1e3, float(np.mean(dec_ms)) / 1e3
    b_enc, b_dec = 49 * n + H + W, W + 13 * n + 49 * n
    # the counters' HBM bytes of the encode kernels and of the decode kernels (profiles/pmc_c5.json)
    enc_actual = kernel_traffic_from_profile("c5", n, lambda k: k.startswith("enc_"))
    dec_actual = kernel_traffic_from_profile("c5", n, lambda k: not k.startswith("enc_"))
    gather = ("drp_index_allgather (RCCL) of the 32 B stream stats + index scan" if args.backend == "nccl" else
              "gloo all-gather of the 32 B stream stats + index scan") if dist else "no collective (1 GPU)"
    out_line = {
        "metric": f"round-tripped Change frames/sec (batched encode + decode), {world} MI355X",
        "value": n * world * steps / elapsed, "unit": "frames/s", "n_gpus": world, "steps": steps,
        "warmup": warmup, "ms_per_step": elapsed / steps * 1e3, "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "u8",
        "data": "synthetic: C5 columns + heap generated on device (seeded per rank), resident in HBM",
        "config": {"workload": f"C5: {n} Changes per GPU, 4096 B values, key U[1,256], change/from/to U[0,2^32)",
                   "wire_bytes_per_gpu": W, "heap_bytes_per_gpu": H,
                   "parallelism": f"one stream per GPU, {world} GPU(s); {gather}"},
        "wire_GBps": 2 * W * world * steps / elapsed / 1e9,
        "roofline": {"bound": "hbm", "achieved": (b_enc + b_dec) / (e + d) / 1e9, "peak": HBM_PEAK_GBPS,
                     "unit": "GB/s", "frac": (b_enc + b_dec) / (e + d) / 1e9 / HBM_PEAK_GBPS,
                     "traffic": traffic_from_profile("c5", n), "traffic_source": TRAFFIC_SOURCE % "c5",
                     "kernel": "encode (enc_size, enc_scan, enc_write) + speculative decode",
                     "bytes_model": "encode 49*C + H + W, decode W + 13*F + 49*C (rank 0)"},
        "encode": {"ms": e * 1e3, "GBps": b_enc / e / 1e9, "frac": b_enc / e / 1e9 / HBM_PEAK_GBPS},
        "decode": {"ms": d * 1e3, "GBps": b_dec / d / 1e9, "frac": b_dec / d / 1e9 / HBM_PEAK_GBPS,
                   "frac_kind": "model: the algorithmic bytes W + 13F + 49C over the decode time; the "
                                "claims walk one header per frame and never read the 4 KB values, so "
                                "this is not an HBM fraction (actual_* is)",
                   "actual_GBps": dec_actual / d / 1e9 if dec_actual else None,
                   "actual_frac": dec_actual / d / 1e9 / HBM_PEAK_GBPS if dec_actual else None,
                   "actual_traffic": dec_actual,
                   "exact_fallbacks": t.strict_reruns, "repair_passes": t.spec_repairs,
                   "segmented_repairs": t.seg_repairs, "after_c2": after_c2},
        "encode_actual": {"traffic": enc_actual,
                          "GBps": enc_actual / e / 1e9 if enc_actual else None,
                          "frac": enc_actual / e / 1e9 / HBM_PEAK_GBPS if enc_actual else None},
    }
    if rank == 0 and world == 1 and cpu and not args.no_cpu:
        out_line["cpu_baseline"] = cpu_baseline_c5()
    ctx.close()
    del cols, heap, out, outs, foff
    torch.cuda.empty_cache()
    return out_line if rank == 0 else None


def c2_host(nframes, start, seed):
    """C2 frames in host memory (the layout of c2_on_device)."""
    i = np.arange(start, start + nframes, dtype=np.int64)
    a = np.zeros((nframes, FRAME), np.uint8)
    a[:, 0], a[:, 1], a[:, 2], a[:, 3] = 85, 1, 0x12, 10
    for k in range(10):
        a[:, 4 + k] = 48 + (i // 10 ** (9 - k)) % 10
    a[:, 14], a[:, 15], a[:, 16], a[:, 17] = 0x18, (i % 100) + 1, 0x20, i % 128
    a[:, 18], a[:, 19], a[:, 20], a[:, 21] = 0x28, (i + 1) % 128, 0x32, 64
    a[:, 22:] = np.random.default_rng(seed).integers(0, 256, size=(nframes, 64), dtype=np.uint8)
    return a.reshape(-1)


C3_UNIT_FRAMES, C3_BLOB = 1000, 1 << 20


def c3_host(units, seed=3):
    """C3 (BASELINE configs[2]): units of [1000 C2 frames + one 1 MiB blob], so C2
    frames straddle the blobs' 64 KiB chunk edges; returns the wire as a numpy array."""
    hdr = bytes([(C3_BLOB + 1) & 0x7F | 0x80, ((C3_BLOB + 1) >> 7) & 0x7F | 0x80, (C3_BLOB + 1) >> 14, 2])
    unit = C3_UNIT_FRAMES * FRAME + len(hdr) + C3_BLOB
    out = np.empty(units * unit, np.uint8)
    rng = np.random.default_rng(seed)
    for u in range(units):
        o = u * unit
        out[o:o + C3_UNIT_FRAMES * FRAME] = c2_host(C3_UNIT_FRAMES, u * C3_UNIT_FRAMES, seed + u)
        b = o + C3_UNIT_FRAMES * FRAME
        out[b:b + len(hdr)] = np.frombuffer(hdr, np.uint8)
        out[b + len(hdr):o + unit] = rng.integers(0, 256, size=C3_BLOB, dtype=np.uint8)
    return out


def cpu_baseline_c3(units=16, min_seconds=10.0):
    """The C restatement of decode.js (oracle/, 1 thread) over a C3 sample in 64 KiB writes."""
    O, _ = _oracle_modules()
    wire = c3_host(units, seed=5).tobytes()
    nf = units * (C3_UNIT_FRAMES + 1)
    outs = O.alloc_outputs(nf + 16)
    reps, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < min_seconds:
        r = O.decode_batch(wire, chunk=65536, outs=outs)
        assert r["nframes"] == nf
        reps += 1
    dt = time.perf_counter() - t0
    return {"value": reps * nf / dt, "unit": "frames/s", "cores": 1, "kind": "port",
            "wire_GBps": reps * len(wire) / dt / 1e9,
            "sample": f"C3 sample of {units} units ({len(wire)} B) decoded {reps}x in 64 KiB writes by "
                      f"oracle/drp_oracle.c, {dt:.1f} s on 1 host core"}


def c3_device_leg(pinned, nf, dev, steps, warmup):
    """The C3 wire resident in HBM, decoded by drp_decode_device: the mean decode time (ms)."""
    wd = pinned.to(dev)
    so = torch.tensor([0, wd.numel()], dtype=torch.int64, device=dev)
    cap = nf + 64
    outs = alloc_outputs(cap, dev)
    res = torch.zeros(C.sizeof(drp_amd.StreamResult), dtype=torch.uint8, device=dev)
    ctx = drp_amd.Ctx(dev.index)
    for _ in range(max(1, warmup)):
        ctx.decode_device(wd, so, None, outs, cap, res)
    r = drp_amd.StreamResult.from_buffer_copy(res.cpu().numpy().tobytes())
    assert (r.frames, r.err_code, r.consumed) == (nf, 0, wd.numel()), (r.frames, r.err_code)
    ms = []
    for _ in range(steps):
        ctx.decode_device(wd, so, None, outs, cap, res)
        ms.append(ctx.timing().total_ms)
    ctx.close()
    del wd, outs, res
    torch.cuda.empty_cache()
    return float(np.mean(ms))


def run_c3(args, dev, steps, warmup, cpu, dump=None):
    """C3 through the host-batch path: a ~1 GiB C3 stream in pinned host memory decoded by
    drp_decode_batch (what the Node addon runs per batch) with blob skipping: only the pieces
    around the blobs' headers are staged into HBM, the blob payloads stay in host memory as
    pass-through ranges (decode.js:179-202 only slices them). One step = one decode of the whole
    stream, host columns out. Reports the staged bytes and the H2D time apart. A large pinned batch
    is decoded as it lands (drp_api.hip pipe_chunk: one piece per 128 MiB chunk, hidden behind the
    PCIe copy but for the last), so the roofline prices the device kernels on their own: the same
    wire resident in HBM, decoded in one launch sequence per step (args.c3_leg "device": that leg
    only, for the PMC passes of scripts/gpu_pmc.sh). That leg is a run of its own, so it and the
    roofline are part of --full (or of --c3-leg device) only. dump: the last timed step's host
    columns and counters are written there."""
    units = args.c3_units
    host = c3_host(units)
    pinned = torch.empty(host.size, dtype=torch.uint8, pin_memory=True)
    pinned.numpy()[:] = host
    wire = pinned.numpy()
    del host
    nf = units * (C3_UNIT_FRAMES + 1)
    nc = units * C3_UNIT_FRAMES
    b_dev = wire.size + 13 * nf + 49 * nc
    kern = c3_device_leg(pinned, nf, dev, steps, warmup) if args.full or args.c3_leg == "device" else None
    if args.c3_leg == "device":
        return {"value": 0.0, "roofline_kernel_ms": kern,
                "config": {"workload": f"C3: {units} units, HBM-resident decode only", "frames": nf}}
    outs = drp_amd.alloc_host_outputs(nf + 64)
    ctx = drp_amd.Ctx(dev.index)
    for _ in range(max(1, warmup)):  # (the first batch learns that the stream is blob-heavy)
        r = ctx.decode_batch(wire, outs=outs)
    assert (r["nframes"], r["err_code"], r["consumed"]) == (nf, 0, wire.size), (r["nframes"], r["err_code"])
    ty = r["type"]
    assert int((ty == 1).sum()) == nc and int((ty == 2).sum()) == units
    assert np.array_equal(r["payload_len"][ty == 2], np.full(units, C3_BLOB, np.uint32))
    t_step, t_dec, t_h2d, t_d2h, staged, skipped = [], [], [], [], 0, 0
    for _ in range(steps):
        t0 = time.perf_counter()
        r = ctx.decode_batch(wire, outs=outs)
        t_step.append(time.perf_counter() - t0)
        t = ctx.timing()
        t_dec.append(t.total_ms)
        t_h2d.append(t.h2d_ms)
        t_d2h.append(t.d2h_ms)
        staged, skipped = int(t.h2d_bytes), int(t.h2d_skipped)
    ctx.close()
    if dump:
        counters = ["nframes", "err_frame", "err_code", "err_detail", "consumed", "tail", "blob_remaining"]
        dump_outputs(dump, {k: v for k, v in r.items() if isinstance(v, np.ndarray)}, r["nframes"],
                     [[r[k] for k in counters]])
    step_s = float(np.mean(t_step))
    line = {
        "value": nf / step_s, "unit": "frames/s", "steps": steps, "warmup": warmup, "ms_per_step": step_s * 1e3,
        "data": "synthetic: C3 generator (seeded), in pinned host memory (the Node path's input side)",
        "config": {"workload": f"C3: {units} units of [1000 C2 frames + one 1 MiB blob], one "
                               f"{wire.size / 2**30:.2f} GiB host stream, drp_decode_batch with blob skipping",
                   "wire_bytes": int(wire.size), "frames": nf},
        "wire_GBps": wire.size / step_s / 1e9,
        "h2d": {"staged_bytes": staged, "staged_frac": staged / wire.size, "skipped_bytes": skipped,
                "ms": float(np.mean(t_h2d))},
        "d2h_ms": float(np.mean(t_d2h)),
        "pieces_decode_ms": float(np.mean(t_dec)),
    }
    if kern is not None:
        dec_s = kern / 1e3
        line["roofline"] = {
            "bound": "hbm", "achieved": b_dev / dec_s / 1e9, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
            "frac": b_dev / dec_s / 1e9 / HBM_PEAK_GBPS, "traffic": traffic_from_profile("c3", nf),
            "traffic_source": TRAFFIC_SOURCE % "c3",
            "kernel": "the decode of the same wire resident in HBM (claims + verify + emit, one launch "
                      "sequence, HIP events on libdrp's stream); the host path's pieces "
                      "(pieces_decode_ms, summed with the host waits between their passes) overlap the "
                      "PCIe copy", "kernel_ms": kern,
            "bytes_model": "wire + 13*frames + 49*changes"}
    if cpu:
        line["cpu_baseline"] = cpu_baseline_c3()
    del pinned, wire, outs
    return line


def run_decode(args, dev, rank, world, workload, steps, warmup, dump=None):
    """C2 (one 8.6 GB stream per GPU) or C4 (8192 independent streams sharded over the ranks):
    `steps` timed decodes after `warmup`, each followed for N > 1 by the all-gather of the 32 B
    per-stream stats and the global index scan. Returns rank 0's line (no CPU legs). dump: rank 0
    writes the last timed step's frame table and stream results there."""
    dist = world > 1
    if workload == "c2":
        nframes = args.frames
        wire = c2_on_device(nframes, seed=1234 + rank, dev=dev)
        stream_off = torch.tensor([0, wire.numel()], dtype=torch.int64, device=dev)
        counts, (lo, _) = np.array([nframes]), (rank, rank + 1)
        nstreams_total = world
    else:
        wire, stream_off, counts, (lo, _) = c4_on_device(args.streams, rank, world, dev)
        nframes = int(counts.sum())
        nstreams_total = args.streams
    nlocal = stream_off.numel() - 1
    cap = nframes + 64
    outs = alloc_outputs(cap, dev)
    res = torch.zeros(nlocal * C.sizeof(drp_amd.StreamResult), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)

    ctx = drp_amd.Ctx(dev.index, tile=args.tile)
    state = {"base": None}

    def step():
        ctx.decode_device(wire, stream_off, None, outs, cap, res)
        if dist:  # the only collective: all-gather of 32-byte per-stream stats
            stats = drp_dist.local_stats_device(ctx, res, stream_off)
            if args.backend == "nccl":  # libdrp's RCCL communicator over xGMI (drp_index_allgather)
                _, state["base"] = drp_dist.global_index_rccl(ctx, stats, nstreams_total)
            else:  # gloo rehearsal of several ranks on one GPU
                table = drp_dist.gather_stats(stats, nstreams_total)
                state["base"] = drp_dist.global_index_device(ctx, table)

    for _ in range(max(1, warmup)):
        step()
    if workload == "c2":
        verify_c2(outs, res, nframes, dev)
    else:
        verify_c4(outs, res, counts, state["base"], lo, dev)

    ext = torch.cuda.ExternalStream(ctx.stream, device=dev)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if dist:
        torch.distributed.barrier()
    torch.cuda.synchronize(dev)
    dec_ms, fallbacks, repairs, relisted = [], 0, 0, 0
    t0 = time.perf_counter()
    ev0.record(ext)
    with torch.cuda.stream(ext):  # (torch's stream is libdrp's: no cross-stream waits per decode)
        for _ in range(steps):
            step()
            t = ctx.timing()
            dec_ms.append(t.decode_ms)
            fallbacks += t.strict_reruns
            repairs += t.spec_repairs
            relisted += t.verify_relisted
    ev1.record(ext)
    torch.cuda.synchronize(dev)
    if dist:
        torch.distributed.barrier()
    elapsed = time.perf_counter() - t0
    ev_ms = ev0.elapsed_time(ev1)
    frames_all = torch.tensor([float(nframes)], dtype=torch.float64, device=dev)
    if dist:
        cdev = dev if args.backend == "nccl" else torch.device("cpu")
        tt = torch.tensor([elapsed], dtype=torch.float64, device=cdev)
        torch.distributed.all_reduce(tt, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(tt.item())
        frames_all = frames_all.to(cdev)
        torch.distributed.all_reduce(frames_all)
    frames_node = int(frames_all.item())
    if dump and rank == 0:
        dump_outputs(dump, outs, nframes, stream_results(res))
    ctx.close()
    del wire, outs, res
    torch.cuda.empty_cache()
    if rank != 0:
        return None

    frames_total = frames_node * steps
    wire_total = frames_node * FRAME * steps
    ms_per_step = elapsed / steps * 1e3
    dec_avg_s = float(np.mean(dec_ms)) / 1e3
    b_dec = nframes * FRAME + 13 * nframes + 49 * nframes  # W + 13F + 49C, this GPU
    achieved = b_dec / dec_avg_s / 1e9
    tile = args.tile or 8192
    exact = os.environ.get("DRP_DECODE") == "exact"
    kname = f"decode_tiles<{tile // 64}>" if exact else DECODE_PATH
    gather = ("; drp_index_allgather (RCCL) of 32 B stream stats + index scan" if args.backend == "nccl" else
              "; gloo all-gather of 32 B stream stats + index scan") if dist else "; no collective (1 GPU)"
    if workload == "c2":
        config = {"workload": f"C2: {nframes / 1e6:g}M Change frames x 86 B (64 B values), one "
                              f"{nframes * FRAME / 1e9:.2f} GB stream per GPU",
                  "frames_per_gpu": nframes, "wire_bytes_per_gpu": nframes * FRAME,
                  "parallelism": f"replicas: one stream per GPU, {world} GPU(s){gather}"}
    else:
        config = {"workload": f"C4: {nstreams_total} independent streams of U[8192,16384] C2 frames, "
                              f"contiguous shards over {world} GPU(s)",
                  "frames_node": frames_node, "streams": nstreams_total,
                  "parallelism": f"stream shards, {world} GPU(s){gather}"}
    config["tile_bytes"] = tile
    return {
        "metric": "decoded Change frames/sec + wire GB/s (whole node) at 1/2/4/8 MI355X",
        "value": frames_total / elapsed,
        "unit": "frames/s",
        "n_gpus": world,
        "steps": steps,
        "warmup": warmup,
        "ms_per_step": ms_per_step,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u8",
        "data": "synthetic: C2-shaped generator on device (seeded), resident in HBM before timing",
        "config": config,
        "wire_GBps": wire_total / elapsed / 1e9,
        "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                     "frac": achieved / HBM_PEAK_GBPS, "traffic": traffic_from_profile(workload, nframes),
                     "traffic_source": TRAFFIC_SOURCE % workload,
                     "kernel": kname, "kernel_ms": dec_avg_s * 1e3,
                     "exact_fallbacks": fallbacks, "repair_passes": repairs,
                     "verify_relisted_tiles": relisted // max(1, steps),
                     "bytes_per_launch": b_dec,
                     "bytes_model": "W + 13*frames + 49*changes (86+13+49 = 148 B/frame)"},
        "step_ms_hip_events": ev_ms / steps,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10, help="timed steps (at least 1)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--full", action="store_true",
                    help="also the c4/c5/c3 sub-lines, the CPU baselines, the H2D rate, the Node path, C5's "
                         "decode-after-C2 leg and C3's HBM-resident roofline leg (a plain run: the timed steps only)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the last timed step computed as DIR/<name>.npy (see dump_outputs)")
    ap.add_argument("--frames", type=int, default=100_000_000, help="C2 frames per GPU")
    ap.add_argument("--workload", choices=["c2", "c3", "c4", "c5"], default="c2")
    ap.add_argument("--c5-changes", type=int, default=1_000_000, help="C5 Changes per step")
    ap.add_argument("--streams", type=int, default=8192, help="C4 streams across all GPUs")
    ap.add_argument("--sub-steps", type=int, default=5, help="timed steps of the c4/c5 sub-lines")
    ap.add_argument("--no-sub", action="store_true", help="--full, C2 only: no c3/c4/c5 sub-lines")
    ap.add_argument("--c3-units", type=int, default=947, help="C3 units (1000 C2 frames + 1 MiB blob) per step")
    ap.add_argument("--c3-leg", choices=["both", "device"], default="both",
                    help="c3: device = only the HBM-resident decode (the PMC passes)")
    ap.add_argument("--tile", type=int, default=0)
    ap.add_argument("--no-cpu", action="store_true", help="--full: no CPU baselines, H2D rate or Node path")
    ap.add_argument("--no-after-c2", action="store_true",
                    help="--full, C5: no decode-after-C2 leg (PMC passes: its C2 kernels would join C5's counters)")
    ap.add_argument("--backend", default="nccl", help="nccl (RCCL) for runs; gloo only to rehearse "
                    "several ranks on one GPU")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if os.environ.get("DRP_BENCH_WATCHDOG"):  # (hang finding: every thread's Python stack, then exit)
        import faulthandler
        faulthandler.dump_traceback_later(float(os.environ["DRP_BENCH_WATCHDOG"]), exit=True)

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # one process per GPU: re-launch under torch.distributed.run before anything touches
        # the GPU (this process never initialises HIP), and exit with its status
        import socket
        import subprocess
        with socket.socket() as so:
            so.bind(("127.0.0.1", 0))
            port = so.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", f"--master-port={port}", os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.call(cmd))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: launch one rank per GPU")
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dist = world > 1
    if dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            torch.distributed.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            torch.distributed.init_process_group(args.backend)
    dev = torch.device("cuda", local % max(1, torch.cuda.device_count()))
    torch.cuda.set_device(dev)
    cpu = args.full and world == 1 and rank == 0 and not args.no_cpu
    dump = args.dump_outputs

    if args.workload == "c5":
        out = run_c5(args, dev, rank, world, cpu=cpu, dump=dump)
    elif args.workload == "c3":
        out = run_c3(args, dev, args.steps, args.warmup, cpu, dump=dump)
    else:
        out = run_decode(args, dev, rank, world, args.workload, args.steps, args.warmup, dump=dump)
        if cpu:
            if args.workload == "c2":
                out["cpu_baseline"] = cpu_baseline()
                out["cpu_baseline_all_cores"] = cpu_baseline_streams()
            else:
                out["cpu_baseline"] = cpu_baseline_streams()
        if args.full and args.workload == "c2" and not args.no_sub:
            # BASELINE configs[3] and [4] as sub-lines of the same run (own timing, roofline and
            # CPU baseline); the top-level value stays C2's
            c4 = run_decode(args, dev, rank, world, "c4", args.sub_steps, args.warmup)
            c5 = run_c5(args, dev, rank, world, steps=args.sub_steps, warmup=args.warmup, cpu=cpu)
            c3 = run_c3(args, dev, args.sub_steps, args.warmup, cpu)  # (per rank, no collective)
            if rank == 0:
                if cpu:
                    c4["cpu_baseline"] = out["cpu_baseline_all_cores"]
                for k in ("metric", "higher_is_better", "scaling", "vs_baseline", "dtype", "n_gpus"):
                    c4.pop(k, None)
                    c5.pop(k, None)
                out["c4"], out["c5"], out["c3"] = c4, c5, c3
        if cpu:
            out["h2d"] = h2d_rate(dev)
            if args.workload == "c2":
                out["node_path"] = node_path()
    if rank == 0:
        print(json.dumps(out), flush=True)
    drp_dist.close_comms()
    if dist:
        torch.distributed.destroy_process_group()


TRAFFIC_SOURCE = ("not measured in this run: profiles/pmc_%s.json (rocprofv3 FETCH_SIZE x2 + WRITE_SIZE per "
                  "frame over the path's kernels, separate --pmc passes of scripts/gpu_pmc.sh) x this launch's "
                  "frames; null when that summary was measured on other kernel sources (code_hash)")


DECODE_SOURCES = ["drp_api.hip", "drp_decode_spec.hip", "drp_walk.hip", "drp_spec.h", "drp_device.h", "drp_kernels.h",
                  "drp_encode.hip", "drp_keys.hip"]


def decode_code_hash():
    """Hash of the kernel sources of the measured path: a PMC summary is used only for the code
    it was measured on."""
    import hashlib
    h = hashlib.sha256()
    for f in DECODE_SOURCES:
        with open(os.path.join(ROOT, "dat-replication-protocol_amd", "csrc", f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def traffic_from_profile(workload, nframes):
    """HBM bytes per launch from the committed rocprofv3 PMC summary of this workload's decode
    path (profiles/pmc_<workload>.json: FETCH_SIZE x2 + WRITE_SIZE per frame summed over the
    path's kernels, guide §HBM), times this launch's frames; None when no such summary exists
    (a per-frame figure of one workload is never applied to another) or when it was measured on
    other kernel sources (its code_hash differs from decode_code_hash())."""
    p = os.path.join(ROOT, "profiles", f"pmc_{workload}.json")
    try:
        with open(p) as f:
            d = json.load(f)
    except (OSError, ValueError):
        return None
    if d.get("code_hash") != decode_code_hash():
        return None
    return d["hbm_bytes_per_frame"] * nframes if d.get("hbm_bytes_per_frame") else None


def kernel_traffic_from_profile(workload, nframes, select):
    """HBM bytes per launch of the kernels `select` picks from profiles/pmc_<workload>.json's
    per-kernel FETCH_SIZE x2 + WRITE_SIZE figures (same staleness rule as traffic_from_profile)."""
    p = os.path.join(ROOT, "profiles", f"pmc_{workload}.json")
    try:
        with open(p) as f:
            d = json.load(f)
    except (OSError, ValueError):
        return None
    if d.get("code_hash") != decode_code_hash() or not d.get("per_kernel"):
        return None
    b = sum(v.get("fetch_B_per_frame", 0) + v.get("write_B_per_frame", 0) for k, v in d["per_kernel"].items()
            if select(k))
    return b * nframes if b else None


if __name__ == "__main__":
    main()
