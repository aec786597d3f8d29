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

  fan-out     (--fanout-out) drp_fanout_device over the same decoded rows with K = 1, 8, 64 filters
              change >= m_f (m_f spread over the stream's 1..100) against K back-to-back
              drp_select_device calls, alternating, HIP events, the device leg's warm-up and
              repeat counts; one K = 64 run of 64 distinct 8-byte key prefixes (the byte
              conditions); and on the host batch drp_fanout_staged with K = 16 against 16
              drp_relay_staged calls over the same staged batch, alternating, wall clock, with a
              check that the bytes are the same. Written to --fanout-out as its own JSON line.

  latest      (--latest-out) the latest-per-key compaction. Device: --frames decoded C2-shaped rows
              whose keys repeat, three key pools (frames / 16 keys, frames / 1024 keys, and frames / 16
              keys with one hot key on 10 % of the rows); drp_latest_device against drp_select_device
              with the same (NULL) filter, alternating, HIP events, the device leg's warm-up and
              repeat counts; the winners checked against a numpy sort of (key, change, row). Host:
              a --host-mib batch of the frames / 16 stream, staged once per pair, (a) drp_decode_fetch +
              grouping in numpy (lexsort over key hash / change / row, the groups' bytes verified) +
              drp_encode_batch against (b) drp_latest_staged, alternating, wall clock, the bytes
              checked to be the same. Written to --latest-out as its own JSON line. With
              --latest-only the relay and fan-out legs are left out (a run under a kernel trace).

  fan-out of latest  (--fanout-latest-out, default profiles/relay/fanout_latest_bench.json) Device: the
              latest leg's frames / 16 key pool, K = 1, 8, 64 filters change <= 1 + floor(100 f / K)
              (every peer at its own version); one drp_fanout_latest_device against K back-to-back
              drp_latest_device calls, alternating call by call, HIP events, the device leg's warm-up
              and repeat counts; every output's winners checked against a numpy sort of (key, change,
              row). Host: K = 16 over the --host-mib batch, drp_fanout_latest_staged against 16
              drp_latest_staged calls over the same staged batch, alternating, wall clock, the bytes
              checked to be the same. With --fanout-latest-only every other leg is left out.

  store       (--store-out, default profiles/relay/store_bench.json) The latest leg's frames / 16 keyed
              stream, decoded once, as 8 equal batches of rows merged one after the other into an empty
              store (drp_store_merge_device), HIP events around every merge, one warm-up sequence and
              --store-seqs timed ones; per batch also drp_latest_device alone over the same rows (the
              merge's first step) and over the rows of all batches so far (what a hub without a store
              would run), alternating with the merges; then the catch-up (drp_fanout_device over the
              store's view, n = max_keys, and drp_encode_device with the arena as the heap: what
              Store.fanout composes) for K = 1, 8, 64 peers at change > floor(100 f / K), and
              drp_store_compact. The final store is checked against latest_winners. With --store-only
              every other leg is left out. --store-baseline-out: only the drp_latest_device timings
              over the same batches, through nothing the store added, so that they can be taken with
              another commit's library and binding (DRP_LIB, DRP_PY); --store-baseline reads such a
              file into the result.

  digest      (--digest-out, default profiles/relay/digest_bench.json) Two compacted stores: the store
              leg's final store (frames / 16 keys, 74-byte payloads) and one of 65,536 keys with 4 KB
              values. Per store, HIP events, three warm-up rounds and --iters timed ones:
              drp_digest_device over the view (n = max_keys) at bits 8, 12 and 16; against a peer whose
              `change` is raised on 0.1 % and on 10 % of the keys, drp_digest_diff_device,
              drp_select_buckets_device and drp_encode_device at bits 16 (what Store.reconcile composes),
              the rows checked to hold every altered key; and the two yardsticks: drp_store_compact of
              the same store and the full snapshot (drp_fanout_device with one all-pass filter and
              drp_encode_device). --digest-baseline-out: only the yardsticks, through nothing the digest
              added, so that they can be taken with the parent commit's library and binding (DRP_LIB,
              DRP_PY); --digest-baseline reads such a file, and the ratios (digest / compact, reconcile /
              snapshot) are then over the parent's figures. With --digest-only every other leg is left out.

  digest refine  (--digest-refine-out, default profiles/relay/digest_refine_bench.json; no other leg runs)
              The digest leg's two stores and altered shares. The single-level reconcile at bits 16
              (digest, diff, bucket select, encode), then per sub_bits in 2, 4, 8:
              drp_digest_refine_device, drp_digest_diff_cells_device, drp_select_refined_device and
              drp_encode_device, the rows out (checked to hold every altered key) and the bytes one hub
              sends: first-level cells, cells2 and frames. A probe of the refine's LDS copy of the cells
              (every row a member of 256 .. 4096 cells). --digest-refine-baseline-out: the yardsticks
              and the single-level reconcile only, to be taken with the parent commit's library and
              binding (DRP_LIB, DRP_PY); --digest-refine-baseline reads such a file, and the ratios are
              then over the parent's figures.

  order       (--order-out, default profiles/relay/order_bench.json; no other leg runs) The store leg's
              final store and its catch-up shapes K = 1, 8, 64. Per shape, HIP events, three warm-up
              rounds and --iters timed ones: drp_fanout_device and drp_encode_device over all rows (the
              yardstick), drp_order_device alone, the same with limit = 1000 per peer and the encode of
              those pages, drp_order_device with every pass left on (a second ctx opened under
              DRP_ORDER_SKIP=0), and both again over uniform 64-bit keys in the same rows. Every timed
              call's output is checked once against numpy's stable argsort per segment.
              --order-baseline-out: only the yardstick, to be taken with the parent commit's library
              and binding (DRP_LIB, DRP_PY); --order-baseline reads such a file, and the ratio order /
              encode is then also given over the parent's figure. --order-profile: K = 64 and the plain
              calls alone, for a rocprofv3 --kernel-trace --stats run (profiles/relay/order_kernel_stats.csv).

  keyorder    (--keyorder-out, default profiles/relay/keyorder_bench.json; no other leg runs) The store
              leg's final store, listed in key order as K = 1 and K = 64 version-bounded listings that
              share its rows out among them, over its own keys and over the same keys behind a shared 16-byte prefix (a
              second heap built here). HIP events, three warm-up rounds and --iters timed ones:
              drp_order_keys_device whole, the same with limit 0 for every peer (prepass, sort and cut:
              no gather), and drp_order_device over the same rows with every pass left on (a second ctx
              opened under DRP_ORDER_SKIP=0): both share the pass kernels, so time per active digit
              pass is compared. The host alternative: the keys copied to the host and sorted there
              with numpy's stable argsort, per segment, on one core (wall clock, copy included). The
              K = 1 permutation is checked against that argsort. Launches and active passes are
              computed here from the keys by the launcher's rule; the call waits for the stream once.

  news        (--news-out, default profiles/relay/news_bench.json; no other leg runs) The store leg's
              stream and sequences of 8 merges into an empty store, three ways: drp_store_merge_device,
              drp_store_merge_report_device with a NULL report, and with a full report (outcome,
              news_type with KEEP_BLOBS, reply with reply_cap = the batch's rows). Then the hub step
              over batch 0 for K = 1, 8, 64 all-pass peers (the merge with its news column,
              drp_fanout_device over the news view, drp_encode_device: what Store.relay_news composes)
              with 0 %, 10 % and 100 % of the batch's winners news to the store (the store holds the
              batch; holds it but for a raised `change` on every tenth key; is empty), a fresh store
              before every timed round, against relaying the whole batch (drp_fanout_device and
              drp_encode_device over all its rows); times and bytes out. --news-baseline-out: the plain
              merge sequences and the whole-batch relay only, to be taken with the parent commit's
              library and binding (DRP_LIB, DRP_PY); --news-baseline reads such a file, and the result
              says per batch whether this build's medians lie inside the parent's own min-max spread.

  lookup      (--lookup-out, default profiles/relay/lookup_bench.json; no other leg runs) The store leg's
              merge sequences (timed again: the merge shares its probe with the lookup) and its final
              store. HIP events, three warm-up rounds and --iters timed ones: drp_store_lookup_device
              over 64, 65,536 and 1.25M keys laid end to end (columns built here, no wire), half of
              them held: the verdicts alone, the multi-get (every found row emitted) and the
              drp_encode_device of its rows, every hit row checked to hold the queried key; then a
              have-list of every key at change 50 with lack_type, and the drp_select_device and
              drp_encode_device over the store's view under that column (what Store.sync_reply
              composes). --lookup-baseline-out: the merge sequences and what the parent commit can do
              for a point read (one drp_fanout_device over the store with the 64 keys as 64
              DRP_SEL_KEY_PREFIX filters, and the encode), to be taken with the parent commit's
              library and binding (DRP_LIB, DRP_PY); --lookup-baseline reads such a file, and the
              result says per batch whether this build's merge medians lie inside the parent's own
              min-max spread.

  lifecycle   (--lifecycle-out, default profiles/relay/lifecycle_bench.json; no other leg runs) The
              store leg's final store (its key count, compacted) and its view as the batch. HIP events,
              three warm-up rounds and --runs timed ones, medians: (a) drp_store_init and
              drp_store_merge_device of the view into a fresh store, the only way to move a store
              without the lifecycle calls; (b) drp_store_init and drp_store_load_device of the same
              view, without and with clash, the loaded store checked to equal the merged one byte for
              byte; (c) drp_store_rehash_device of the final store, without and with report; (d)
              drp_store_compact and drp_store_init alone, for scale. All in one run, one library.

Prints one JSON line (and writes it to --out). Needs an MI355X: there is no CPU path.

  hipcc -O3 --offload-arch=gfx950 scripts/probe_bw.hip -o exp/probe_bw
  python scripts/bench_relay.py --probe exp/probe_bw --out profiles/relay/relay_bench.json \\
      --fanout-out profiles/relay/fanout_bench.json
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
# (DRP_PY: another commit's binding directory, with DRP_LIB naming that commit's library: an A/B)
sys.path.insert(0, os.environ.get("DRP_PY") or os.path.join(ROOT, "dat-replication-protocol_amd", "python"))

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


def device_setup(ctx, drp_amd, torch, S, frames, wire=None):
    """frames C2 frames (or the given wire of as many frames) resident in HBM and decoded:
    (wire_t, cols, n)."""
    dev = torch.device("cuda", 0)
    if wire is None:
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
    return wire_t, cols, n


def device_leg(ctx, drp_amd, torch, decoded, iters):
    dev = torch.device("cuda", 0)
    wire_t, cols, n = decoded
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


def _stat(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}


def _row_tensors(torch, dev, room):
    return {k: torch.zeros(room, dtype=(torch.int32 if k.endswith("_len") else torch.uint8 if k == "flags"
                                         else torch.int64), device=dev) for k in SRC_KEYS}


def fanout_device_leg(ctx, drp_amd, torch, decoded, iters):
    """drp_fanout_device with K filters against K back-to-back drp_select_device calls over the
    same decoded rows; the library is called directly (no per-call stream ordering in between)."""
    dev = torch.device("cuda", 0)
    wire_t, cols, n = decoded
    L = ctx.L
    tp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    fr = drp_amd.Frames(tp(cols["payload_off"]), tp(cols["payload_len"]), tp(cols["type"]))
    co = drp_amd.Changes(*[tp(cols[k]) for k in drp_amd.COLS32], tp(cols["change"]), tp(cols["from"]),
                         tp(cols["to"]), tp(cols["flags"]), None)
    ext = ctx._ext(dev)
    one = _row_tensors(torch, dev, n)  # a single select's rows (every call of the sequence reuses them)
    one_src = drp_amd.ChangeSrc(*[tp(one[k]) for k in SRC_KEYS])
    nsel_t = torch.zeros(1, dtype=torch.int64, device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(ext)
        fn()
        e1.record(ext)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def closed_form(m):  # rows with change = i % 100 + 1 >= m
        keep = 100 - m + 1
        return (n // 100) * keep + max(0, n % 100 - (m - 1))

    res = {}
    for K in (1, 8, 64):
        ms = [1 + (f * 100) // K for f in range(K)]
        flt = [drp_amd.make_filter(change_range=(m, 2**64 - 1)) for m in ms]
        arr = drp_amd.filter_array(flt)
        counts = [closed_form(m) for m in ms]
        total = sum(counts)
        many = _row_tensors(torch, dev, total)
        many_src = drp_amd.ChangeSrc(*[tp(many[k]) for k in SRC_KEYS])
        rb_t = torch.zeros(K + 1, dtype=torch.int64, device=dev)

        def fan():
            rc = L.drp_fanout_device(ctx.h, tp(wire_t), wire_t.numel(), C.byref(fr), C.byref(co), n, arr, K,
                                     C.byref(many_src), total, None, tp(rb_t), None)
            assert rc == 0, rc

        def seq():
            for f in flt:
                rc = L.drp_select_device(ctx.h, tp(wire_t), wire_t.numel(), C.byref(fr), C.byref(co), n, C.byref(f),
                                         C.byref(one_src), None, tp(nsel_t))
                assert rc == 0, rc

        tf, ts = [], []
        for it in range(iters + 3):  # (three warm-ups, as the device leg; alternating)
            a, b = timed(fan), timed(seq)
            if it >= 3:
                tf.append(a)
                ts.append(b)
        rb = rb_t.cpu().numpy()
        assert [int(rb[f + 1] - rb[f]) for f in range(K)] == counts, "fan-out counts"
        assert int(nsel_t.cpu()[0]) == counts[-1]
        # the last filter's output against the sequence's last select (the same rows, the same order)
        a0 = int(rb[K - 1])
        for k in ("change", "key_off", "flags"):
            assert bool(torch.equal(many[k][a0:a0 + counts[-1]], one[k][:counts[-1]])), k
        model = n * 10 + (K + 1) * n // 8 * 2 + n * 57 + total * WRITE_B  # count, ballots (written, read), scatter
        res[f"K{K}"] = {"filters": K, "rows_out": total, "fanout_ms": _stat(tf), "sequential_ms": _stat(ts),
                        "sequential_over_fanout": statistics.median(ts) / statistics.median(tf),
                        "ranges_overlap": not (max(tf) < min(ts) or max(ts) < min(tf)),
                        "fanout_model_bytes": model, "fanout_model_TBps": model / statistics.median(tf) / 1e9}
        many = many_src = None  # (tens of GB at K = 64: freed before the next K allocates)
        torch.cuda.empty_cache()
    # the byte conditions: 64 distinct 8-byte key prefixes (each the first 8 of the 10 key digits: 100 rows)
    K = 64
    ps = [(f * (n // 100)) // K for f in range(K)]
    flt = [drp_amd.make_filter(key_prefix=b"%08d" % p) for p in ps]
    arr = drp_amd.filter_array(flt)
    counts = [max(0, min(n, p * 100 + 100) - p * 100) for p in ps]
    total = sum(counts)
    many = _row_tensors(torch, dev, total)
    many_src = drp_amd.ChangeSrc(*[tp(many[k]) for k in SRC_KEYS])
    rb_t = torch.zeros(K + 1, dtype=torch.int64, device=dev)

    def fan_bytes():
        rc = L.drp_fanout_device(ctx.h, tp(wire_t), wire_t.numel(), C.byref(fr), C.byref(co), n, arr, K,
                                 C.byref(many_src), total, None, tp(rb_t), None)
        assert rc == 0, rc

    tb = [timed(fan_bytes) for _ in range(iters + 3)][3:]
    rb = rb_t.cpu().numpy()
    assert [int(rb[f + 1] - rb[f]) for f in range(K)] == counts, "key prefix counts"
    res["K64_key_prefix8"] = {"filters": K, "rows_out": total, "fanout_ms": _stat(tb)}
    res["frames"] = n
    res["iters"] = iters
    return res


def fanout_host_leg(ctx, drp_amd, S, mib, runs, K=16):
    """drp_fanout_staged with K filters against K drp_relay_staged calls over the same staged batch
    (staged once per timed run, outside the timed part: it is the same for both)."""
    L = ctx.L
    nbytes = mib << 20
    wire = S.c2_stream(nbytes // 86 + 1, seed=1)[:nbytes].copy()
    ms = [1 + (f * 100) // K for f in range(K)]
    flt = [drp_amd.make_filter(change_range=(m, 2**64 - 1)) for m in ms]
    arr = drp_amd.filter_array(flt)
    U64, U32 = C.c_uint64, C.c_uint32
    out_f, out_s = np.zeros(K * nbytes, np.uint8), np.zeros(K * nbytes, np.uint8)
    off_f, nsel_f = np.zeros(K + 1, np.uint64), np.zeros(K, np.uint64)

    def stage():
        carry = drp_amd.Carry(0, 0, 0, 0, 0)
        nf, ef, ec, ed = U64(), U64(), U32(), U32()
        rc = L.drp_decode_stage(ctx.h, drp_amd._p(wire), nbytes, C.byref(carry), C.byref(nf), C.byref(ef),
                                C.byref(ec), C.byref(ed))
        assert rc == 0 and ec.value == 0, (rc, ec.value)

    def fan():
        rc = L.drp_fanout_staged(ctx.h, arr, K, drp_amd._p(out_f), out_f.size, drp_amd._p(off_f), drp_amd._p(nsel_f),
                                 None, None, 0, None)
        assert rc == 0, rc

    def seq():
        at, ns = 0, []
        for f in flt:
            written, nsel = U64(), U64()
            rc = L.drp_relay_staged(ctx.h, C.byref(f), drp_amd._p(out_s[at:]), out_s.size - at, C.byref(written),
                                    C.byref(nsel))
            assert rc == 0, rc
            at += int(written.value)
            ns.append(int(nsel.value))
        return at, ns

    tf, ts = [], []
    same = False
    for it in range(runs + 2):  # (two warm-ups; alternating)
        stage()
        t0 = time.perf_counter()
        fan()
        t1 = time.perf_counter()
        at, ns = seq()
        t2 = time.perf_counter()
        if it == 1:
            same = (int(off_f[K]) == at and ns == [int(v) for v in nsel_f] and
                    out_f[:at].tobytes() == out_s[:at].tobytes())
            assert same, (int(off_f[K]), at)
        if it >= 2:
            tf.append((t1 - t0) * 1e3)
            ts.append((t2 - t1) * 1e3)
    return {"batch_bytes": nbytes, "filters": K, "out_bytes": int(off_f[K]), "rows_out": int(nsel_f.sum()),
            "runs": runs, "fanout_staged_ms": _stat(tf), "sequential_relay_ms": _stat(ts),
            "sequential_over_fanout": statistics.median(ts) / statistics.median(tf),
            "ranges_overlap": not (max(tf) < min(ts) or max(ts) < min(tf)), "same_bytes": same}


# ---- latest per key ---------------------------------------------------------------------------

def keyed_c2_stream(key_ids, seed=1):
    """_streams.c2_stream's 86-byte frames with row i's key the 10 digits of key_ids[i]: change =
    i % 100 + 1 (so a key's rows tie now and then), from = i % 128, to = (i + 1) % 128, 64 random
    value bytes."""
    n = len(key_ids)
    i = np.arange(n, dtype=np.int64)
    a = np.zeros((n, 86), np.uint8)
    a[:, 0], a[:, 1], a[:, 2], a[:, 3] = 85, 1, 0x12, 10
    for k in range(10):
        a[:, 4 + k] = 48 + (key_ids // 10 ** (9 - k)) % 10
    a[:, 14], a[:, 15] = 0x18, (i % 100) + 1
    a[:, 16], a[:, 17] = 0x20, i % 128
    a[:, 18], a[:, 19] = 0x28, (i + 1) % 128
    a[:, 20], a[:, 21] = 0x32, 64
    a[:, 22:] = np.random.default_rng(seed).integers(0, 256, size=(n, 64), dtype=np.uint8)
    return a.reshape(-1)


def latest_pools(n, seed=7):
    """The three key pools of the device leg: name -> key id of every row."""
    rng = np.random.default_rng(seed)
    p16 = rng.integers(0, max(1, n // 16), n, dtype=np.int64)
    hot = p16.copy()
    hot[rng.random(n) < 0.10] = 0
    return {"keys_n_over_16": p16, "keys_n_over_1024": rng.integers(0, max(1, n // 1024), n, dtype=np.int64),
            "hot_key_10pct": hot}


def latest_winners(key_ids):
    """Per key the row with the greatest (change, row), change = row % 100 + 1: rows, increasing."""
    n = len(key_ids)
    assert n < 1 << 25 and int(key_ids.max()) < 1 << 31
    i = np.arange(n, dtype=np.int64)
    packed = np.sort((key_ids << 32) | ((i % 100 + 1) << 25) | i)
    last = np.flatnonzero(np.append(packed[1:] >> 32 != packed[:-1] >> 32, True))
    return np.sort(packed[last] & ((1 << 25) - 1))


def latest_device_leg(ctx, drp_amd, torch, frames, iters):
    dev = torch.device("cuda", 0)
    L = ctx.L
    tp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    res = {"frames": frames, "iters": iters}
    for name, key_ids in latest_pools(frames).items():
        wire = keyed_c2_stream(key_ids)
        want = latest_winners(key_ids)
        wire_t, cols, n = device_setup(ctx, drp_amd, torch, None, frames, wire=wire)
        del wire
        fr = drp_amd.Frames(tp(cols["payload_off"]), tp(cols["payload_len"]), tp(cols["type"]))
        co = drp_amd.Changes(*[tp(cols[k]) for k in drp_amd.COLS32], tp(cols["change"]), tp(cols["from"]),
                             tp(cols["to"]), tp(cols["flags"]), None)
        rows = _row_tensors(torch, dev, n)
        src = drp_amd.ChangeSrc(*[tp(rows[k]) for k in SRC_KEYS])
        idx_t = torch.zeros(n, dtype=torch.int64, device=dev)
        nsel_t = torch.zeros(1, dtype=torch.int64, device=dev)
        ext = ctx._ext(dev)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(ext)
            rc = fn(ctx.h, tp(wire_t), wire_t.numel(), C.byref(fr), C.byref(co), n, None, C.byref(src), tp(idx_t),
                    tp(nsel_t))
            e1.record(ext)
            e1.synchronize()
            assert rc == 0, rc
            return e0.elapsed_time(e1)

        tl, ts = [], []
        for it in range(iters + 3):  # (three warm-ups, as the device leg; alternating, the latest call last)
            b, a = timed(L.drp_select_device), timed(L.drp_latest_device)
            if it >= 3:
                tl.append(a)
                ts.append(b)
        nsel = int(nsel_t.cpu()[0])
        assert nsel == len(want), (name, nsel, len(want))
        assert np.array_equal(idx_t[:nsel].cpu().numpy(), want), name
        assert np.array_equal(rows["change"][:nsel].cpu().numpy(), want % 100 + 1), name
        res[name] = {"keys": int(len(np.unique(key_ids))), "winners": nsel, "latest_ms": _stat(tl), "select_ms": _stat(ts),
                     "latest_over_select": statistics.median(tl) / statistics.median(ts),
                     "scratch_bytes": int(n * 8 + 24 * (1 << int(2 * n - 1).bit_length()))}
        print("latest", name, res[name]["latest_ms"], file=sys.stderr, flush=True)
        del wire_t, cols, rows, idx_t
        torch.cuda.empty_cache()
    return res


def _field_hash(wire, off, ln, mult):
    """A u64 hash of wire[off, off + ln) per row (the length and a multiplier per byte position)."""
    h = ln.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    for width in np.unique(ln):
        if width:
            r = np.flatnonzero(ln == width)
            m = wire[off[r][:, None] + np.arange(width, dtype=np.uint64)]
            h[r] += (m.astype(np.uint64) * mult[:width]).sum(axis=1, dtype=np.uint64)
    return h


def _fields_equal(wire, off_a, off_b, ln):
    """wire[off_a, off_a + ln) == wire[off_b, off_b + ln) for every row."""
    for width in np.unique(ln):
        if width:
            r = np.flatnonzero(ln == width)
            k = np.arange(width, dtype=np.uint64)
            if not np.array_equal(wire[off_a[r][:, None] + k], wire[off_b[r][:, None] + k]):
                return False
    return True


def host_latest_rows(wire, host, n):
    """The host grouping path (a) does: the rows to keep, increasing. Per well-formed Change a hash of
    (subset presence, subset bytes, key bytes), a lexsort over (hash, change, row), every group's
    bytes verified against its first row, the last row of every group."""
    cand = np.flatnonzero(((host["type"][:n] & 0x3F) == 1) & ((host["flags"][:n] & 4) == 0))
    po = host["payload_off"][cand]
    has = (host["flags"][cand] & 1).astype(np.uint64)
    koff, klen = po + host["key_off"][cand], host["key_len"][cand]
    soff, slen = po + host["subset_off"][cand], host["subset_len"][cand] * has.astype(np.uint32)
    mult = np.random.default_rng(5).integers(1, 1 << 63, size=int(max(klen.max(), slen.max(), 1)), dtype=np.uint64) | np.uint64(1)
    h = _field_hash(wire, koff, klen, mult) * np.uint64(0xC2B2AE3D27D4EB4F) + _field_hash(wire, soff, slen, mult) + has
    order = np.lexsort((cand, host["change"][cand], h))
    hs = h[order]
    first = np.append(True, hs[1:] != hs[:-1])
    leader = order[np.maximum.accumulate(np.where(first, np.arange(len(order)), 0))]
    assert np.array_equal(has[order], has[leader]) and np.array_equal(klen[order], klen[leader]) and \
        np.array_equal(slen[order], slen[leader]) and _fields_equal(wire, koff[order], koff[leader], klen[order]) and \
        _fields_equal(wire, soff[order], soff[leader], slen[order]), "hash collision"
    return np.sort(cand[order[np.append(first[1:], True)]])


def latest_host_leg(ctx, drp_amd, mib, runs):
    L = ctx.L
    nbytes = mib << 20
    frames = nbytes // 86 + 1
    wire = keyed_c2_stream(latest_pools(frames)["keys_n_over_16"])[:nbytes].copy()
    host = drp_amd.alloc_host_outputs(nbytes // 86 + 8)
    fr, co = drp_amd._structs(host, drp_amd._p)
    out_a, out_b = np.zeros(nbytes, np.uint8), np.zeros(nbytes, np.uint8)
    U64, U32 = C.c_uint64, C.c_uint32

    def stage():
        carry = drp_amd.Carry(0, 0, 0, 0, 0)
        nf, ef, ec, ed = U64(), U64(), U32(), U32()
        rc = L.drp_decode_stage(ctx.h, drp_amd._p(wire), nbytes, C.byref(carry), C.byref(nf), C.byref(ef),
                                C.byref(ec), C.byref(ed))
        assert rc == 0 and ec.value == 0, (rc, ec.value)
        return int(nf.value)

    def path_a(n):
        assert L.drp_decode_fetch(ctx.h, C.byref(fr), C.byref(co), 0, n) == 0
        keep = host_latest_rows(wire, host, n)
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
        written, nsel = U64(), U64()
        rc = L.drp_latest_staged(ctx.h, None, drp_amd._p(out_b), nbytes, C.byref(written), C.byref(nsel))
        assert rc == 0, rc
        return int(written.value), int(nsel.value)

    ta, tb, same = [], [], False
    for it in range(runs + 2):  # (two warm-ups; staged once per pair; (b) first: (a)'s host encode ends the staged batch)
        t0 = time.perf_counter()
        n = stage()
        t1 = time.perf_counter()
        rb = path_b()
        t2 = time.perf_counter()
        ra = path_a(n)
        t3 = time.perf_counter()
        if it == 1:
            same = ra == rb and out_a[:ra[0]].tobytes() == out_b[:rb[0]].tobytes()
            assert same, (ra, rb)
        if it >= 2:  # each path with the stage it needs
            tb.append((t2 - t0) * 1e3)
            ta.append((t1 - t0 + t3 - t2) * 1e3)
    return {"batch_bytes": nbytes, "rows": n, "winners": ra[1], "out_bytes": ra[0], "runs": runs,
            "a_stage_fetch_group_encode_ms": _stat(ta), "b_stage_latest_ms": _stat(tb),
            "a_over_b": statistics.median(ta) / statistics.median(tb), "ranges_overlap": not max(tb) < min(ta),
            "same_bytes": same}


# ---- fan-out of latest per key ------------------------------------------------------------------

def snapshot_winners(key_ids, tmaxes):
    """latest_winners under change <= T for every T of tmaxes: one sort of (key, change, row); the
    rows a T keeps are a prefix of every key's run, so each T takes the last kept row per key."""
    n = len(key_ids)
    assert n < 1 << 25 and int(key_ids.max()) < 1 << 31
    i = np.arange(n, dtype=np.int64)
    packed = np.sort((key_ids << 32) | ((i % 100 + 1) << 25) | i)
    out = []
    for t in tmaxes:
        sub = packed[((packed >> 25) & 127) <= t]
        last = np.flatnonzero(np.append(sub[1:] >> 32 != sub[:-1] >> 32, True))
        out.append(np.sort(sub[last] & ((1 << 25) - 1)))
    return out


def _version_filters(drp_amd, K):
    ts = [1 + (100 * f) // K for f in range(K)]  # every peer at its own version
    return ts, [drp_amd.make_filter(change_range=(0, t)) for t in ts]


def fanout_latest_device_leg(ctx, drp_amd, torch, frames, iters):
    """One drp_fanout_latest_device with K filters against K back-to-back drp_latest_device calls over
    the latest leg's frames / 16 key pool, alternating call by call, HIP events."""
    dev = torch.device("cuda", 0)
    L = ctx.L
    tp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    key_ids = latest_pools(frames)["keys_n_over_16"]
    wire_t, cols, n = device_setup(ctx, drp_amd, torch, None, frames, wire=keyed_c2_stream(key_ids))
    fr = drp_amd.Frames(tp(cols["payload_off"]), tp(cols["payload_len"]), tp(cols["type"]))
    co = drp_amd.Changes(*[tp(cols[k]) for k in drp_amd.COLS32], tp(cols["change"]), tp(cols["from"]),
                         tp(cols["to"]), tp(cols["flags"]), None)
    ext = ctx._ext(dev)
    one = _row_tensors(torch, dev, n)  # a single call's rows (every call of the sequence reuses them)
    one_src = drp_amd.ChangeSrc(*[tp(one[k]) for k in SRC_KEYS])
    one_idx = torch.zeros(n, dtype=torch.int64, device=dev)
    nsel_t = torch.zeros(1, dtype=torch.int64, device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(ext)
        fn()
        e1.record(ext)
        e1.synchronize()
        return e0.elapsed_time(e1)

    res = {"frames": n, "iters": iters, "keys": int(len(np.unique(key_ids)))}
    for K in (1, 8, 64):
        ts_, flt = _version_filters(drp_amd, K)
        arr = drp_amd.filter_array(flt)
        want = snapshot_winners(key_ids, ts_)
        total = sum(len(w) for w in want)
        many = _row_tensors(torch, dev, total)
        many_src = drp_amd.ChangeSrc(*[tp(many[k]) for k in SRC_KEYS])
        many_idx = torch.zeros(total, dtype=torch.int64, device=dev)
        rb_t = torch.zeros(K + 1, dtype=torch.int64, device=dev)

        def fan():
            rc = L.drp_fanout_latest_device(ctx.h, tp(wire_t), wire_t.numel(), C.byref(fr), C.byref(co), n, arr, K,
                                            C.byref(many_src), total, tp(many_idx), tp(rb_t))
            assert rc == 0, rc

        def seq():
            for f in flt:
                rc = L.drp_latest_device(ctx.h, tp(wire_t), wire_t.numel(), C.byref(fr), C.byref(co), n, C.byref(f),
                                         C.byref(one_src), tp(one_idx), tp(nsel_t))
                assert rc == 0, rc

        tf, tq = [], []
        for it in range(iters + 3):  # (three warm-ups; alternating call by call)
            a, b = timed(fan), timed(seq)
            if it >= 3:
                tf.append(a)
                tq.append(b)
        rb = rb_t.cpu().numpy()
        assert [int(rb[f + 1] - rb[f]) for f in range(K)] == [len(w) for w in want], "winners per output"
        idx = many_idx.cpu().numpy()
        ch = many["change"].cpu().numpy()
        for f in range(K):
            a0, a1 = int(rb[f]), int(rb[f + 1])
            assert np.array_equal(idx[a0:a1], want[f]), (K, f)
            assert np.array_equal(ch[a0:a1], want[f] % 100 + 1), (K, f)
        # the sequence's last call against the same numpy side
        assert int(nsel_t.cpu()[0]) == len(want[-1]) and np.array_equal(one_idx[:len(want[-1])].cpu().numpy(), want[-1])
        nslots = 1 << int(2 * n - 1).bit_length()
        res[f"K{K}"] = {"filters": K, "rows_out": total, "fanout_latest_ms": _stat(tf), "sequential_ms": _stat(tq),
                        "sequential_over_fanout_latest": statistics.median(tq) / statistics.median(tf),
                        "ranges_overlap": not (max(tf) < min(tq) or max(tq) < min(tf)),
                        "pass_width": min(K, 8), "passes": -(-K // 8),
                        "group_scratch_bytes": int(n * 8 + nslots * 8 + 2 * ((n + 63) // 64 * 8) + n * 16 * min(K, 8))}
        print("fanout_latest", K, res[f"K{K}"]["fanout_latest_ms"], res[f"K{K}"]["sequential_ms"], file=sys.stderr,
              flush=True)
        many = many_src = many_idx = None
        torch.cuda.empty_cache()
    return res


def fanout_latest_host_leg(ctx, drp_amd, mib, runs, K=16):
    """drp_fanout_latest_staged with K filters against K drp_latest_staged calls over the same staged
    batch (staged once per pair, outside the timed part: it is the same for both), alternating."""
    L = ctx.L
    nbytes = mib << 20
    frames = nbytes // 86 + 1
    wire = keyed_c2_stream(latest_pools(frames)["keys_n_over_16"])[:nbytes].copy()
    _, flt = _version_filters(drp_amd, K)
    arr = drp_amd.filter_array(flt)
    U64, U32 = C.c_uint64, C.c_uint32
    out_f, out_s = np.zeros(K * nbytes, np.uint8), np.zeros(K * nbytes, np.uint8)
    off_f, nsel_f = np.zeros(K + 1, np.uint64), np.zeros(K, np.uint64)

    def stage():
        carry = drp_amd.Carry(0, 0, 0, 0, 0)
        nf, ef, ec, ed = U64(), U64(), U32(), U32()
        rc = L.drp_decode_stage(ctx.h, drp_amd._p(wire), nbytes, C.byref(carry), C.byref(nf), C.byref(ef),
                                C.byref(ec), C.byref(ed))
        assert rc == 0 and ec.value == 0, (rc, ec.value)

    def fan():
        rc = L.drp_fanout_latest_staged(ctx.h, arr, K, drp_amd._p(out_f), out_f.size, drp_amd._p(off_f),
                                        drp_amd._p(nsel_f))
        assert rc == 0, rc

    def seq():
        at, ns = 0, []
        for f in flt:
            written, nsel = U64(), U64()
            rc = L.drp_latest_staged(ctx.h, C.byref(f), drp_amd._p(out_s[at:]), out_s.size - at, C.byref(written),
                                     C.byref(nsel))
            assert rc == 0, rc
            at += int(written.value)
            ns.append(int(nsel.value))
        return at, ns

    tf, tq = [], []
    same = False
    for it in range(runs + 2):  # (two warm-ups; alternating)
        stage()
        t0 = time.perf_counter()
        fan()
        t1 = time.perf_counter()
        at, ns = seq()
        t2 = time.perf_counter()
        if it == 1:
            same = (int(off_f[K]) == at and ns == [int(v) for v in nsel_f] and
                    out_f[:at].tobytes() == out_s[:at].tobytes())
            assert same, (int(off_f[K]), at)
        if it >= 2:
            tf.append((t1 - t0) * 1e3)
            tq.append((t2 - t1) * 1e3)
    return {"batch_bytes": nbytes, "filters": K, "out_bytes": int(off_f[K]), "rows_out": int(nsel_f.sum()),
            "runs": runs, "fanout_latest_staged_ms": _stat(tf), "sequential_latest_staged_ms": _stat(tq),
            "sequential_over_fanout_latest": statistics.median(tq) / statistics.median(tf),
            "ranges_overlap": not (max(tf) < min(tq) or max(tq) < min(tf)), "same_bytes": same}


# ---- store ----------------------------------------------------------------------------------------

STORE_BATCHES = 8


def _store_input(ctx, drp_amd, torch, frames):
    """The keyed stream decoded once; batch b is rows [b m, (b + 1) m) of its columns over the one wire."""
    frames -= frames % STORE_BATCHES
    key_ids = latest_pools(frames)["keys_n_over_16"]
    wire_t, cols, n = device_setup(ctx, drp_amd, torch, None, frames, wire=keyed_c2_stream(key_ids))
    return key_ids, wire_t, cols, n, n // STORE_BATCHES


def _latest_times(ctx, drp_amd, torch, wire_t, cols, n, m, seqs):
    """drp_latest_device alone per batch, and over the rows of all batches so far: [seq][batch] ms."""
    dev = torch.device("cuda", 0)
    L = ctx.L
    tp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    rows = _row_tensors(torch, dev, n)
    src = drp_amd.ChangeSrc(*[tp(rows[k]) for k in SRC_KEYS])
    nsel_t = torch.zeros(1, dtype=torch.int64, device=dev)
    ext = ctx._ext(dev)

    def latest(a, b):
        fr = drp_amd.Frames(tp(cols["payload_off"][a:]), tp(cols["payload_len"][a:]), tp(cols["type"][a:]))
        co = drp_amd.Changes(*[tp(cols[k][a:]) for k in drp_amd.COLS32], tp(cols["change"][a:]), tp(cols["from"][a:]),
                             tp(cols["to"][a:]), tp(cols["flags"][a:]), None)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(ext)
        rc = L.drp_latest_device(ctx.h, tp(wire_t), wire_t.numel(), C.byref(fr), C.byref(co), b - a, None, C.byref(src),
                                 None, tp(nsel_t))
        e1.record(ext)
        e1.synchronize()
        assert rc == 0, rc
        return e0.elapsed_time(e1)

    alone, concat = [], []
    for it in range(seqs + 1):  # (one warm-up sequence)
        ta = [latest(b * m, (b + 1) * m) for b in range(STORE_BATCHES)]
        tc = [latest(0, (b + 1) * m) for b in range(STORE_BATCHES)]
        if it:
            alone.append(ta)
            concat.append(tc)
    return alone, concat, latest


def _per_batch(seq_times):
    return [_stat([t[b] for t in seq_times]) for b in range(STORE_BATCHES)]


def store_baseline(ctx, drp_amd, torch, frames, seqs):
    key_ids, wire_t, cols, n, m = _store_input(ctx, drp_amd, torch, frames)
    alone, concat, _ = _latest_times(ctx, drp_amd, torch, wire_t, cols, n, m, seqs)
    return {"bench": "relay_store_baseline", "frames": n, "batch_rows": m, "seqs": seqs,
            "latest_alone_ms": _per_batch(alone), "latest_concat_ms": _per_batch(concat)}


def store_leg(ctx, drp_amd, torch, frames, seqs, iters):
    dev = torch.device("cuda", 0)
    key_ids, wire_t, cols, n, m = _store_input(ctx, drp_amd, torch, frames)
    keys = int(len(np.unique(key_ids)))
    want = latest_winners(key_ids)
    ext = ctx._ext(dev)
    arena_bytes = 80 * (keys + STORE_BATCHES * m) // 2  # (74-byte payloads; about 0.86 m winners a batch)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(ext)
        fn()
        e1.record(ext)
        e1.synchronize()
        return e0.elapsed_time(e1)

    merges, infos, compacts, store = [], [], [], None
    for it in range(seqs + 1):  # (one warm-up sequence; every sequence starts from an empty store)
        store = None
        torch.cuda.empty_cache()
        store = drp_amd.Store(ctx, keys, arena_bytes)
        tm = []
        for b in range(STORE_BATCHES):
            view = {k: v[b * m:] for k, v in cols.items()}
            tm.append(timed(lambda: ctx.store_merge_device(store, wire_t, view, m)))
            if it == 1:
                infos.append(store.query().as_dict())
        a2 = torch.zeros(store.query().arena_used, dtype=torch.uint8, device=dev)
        before = store.query()
        tc = timed(lambda: ctx.store_compact(store, a2))
        after = store.query()
        assert after.refused == 0 and after.arena_used == before.arena_used - before.arena_dead and after.arena_dead == 0
        store.arena, store.arena_bytes = a2, a2.numel()
        if it:
            merges.append(tm)
            compacts.append(tc)
    # the final store against the numpy side: every key's winner, its change and from
    info = store.query()
    assert info.rows == keys == len(want) and info.refused == 0, (info.rows, keys)
    got = np.sort(store.cols["change"][:keys].cpu().numpy() * 128 + store.cols["from"][:keys].cpu().numpy())
    assert np.array_equal(got, np.sort((want % 100 + 1) * 128 + want % 128)), "store rows"
    alone, concat, _ = _latest_times(ctx, drp_amd, torch, wire_t, cols, n, m, seqs)
    res = {"frames": n, "batches": STORE_BATCHES, "batch_rows": m, "keys": keys, "seqs": seqs,
           "merge_ms": _per_batch(merges), "latest_alone_ms": _per_batch(alone), "latest_concat_ms": _per_batch(concat),
           "merge_info": infos, "compact_ms": _stat(compacts), "compact_live_bytes": int(info.arena_used),
           "arena_bytes": arena_bytes, "table_bytes": int(store.table.numel() * 8)}
    res["merge_over_latest_alone"] = [a["median"] / b["median"] for a, b in zip(res["merge_ms"], res["latest_alone_ms"])]
    res["latest_concat_over_merge"] = [a["median"] / b["median"] for a, b in zip(res["latest_concat_ms"], res["merge_ms"])]
    res["sum_merge_ms"] = sum(a["median"] for a in res["merge_ms"])
    res["sum_latest_alone_ms"] = sum(a["median"] for a in res["latest_alone_ms"])
    res["sum_latest_concat_ms"] = sum(a["median"] for a in res["latest_concat_ms"])
    del wire_t, cols
    torch.cuda.empty_cache()
    # catch-up: what Store.fanout composes, over preallocated outputs
    tp = lambda t: C.c_void_p(t.data_ptr())
    ch = store.cols["change"][:keys].cpu().numpy()
    res["catch_up"] = {}
    for K in (1, 8, 64):
        ts_ = [(100 * f) // K for f in range(K)]
        flt = [drp_amd.make_filter(change_range=(t + 1, 2**64 - 1)) for t in ts_]
        counts = [int((ch > t).sum()) for t in ts_]
        total = sum(counts)
        rows = _row_tensors(torch, dev, total)
        rb_t = torch.zeros(K + 1, dtype=torch.int64, device=dev)
        foff = torch.zeros(total + 1, dtype=torch.int64, device=dev)
        out = torch.zeros(total * 86, dtype=torch.uint8, device=dev)

        def fan():
            ctx.fanout_device(store.arena, store.cols, store.max_keys, flt, rows, total, None, rb_t)

        def enc():
            ctx.encode_device(rows, store.arena, total, foff, out, out.numel())

        tf, te = [], []
        for it in range(iters + 3):
            a, b = timed(fan), timed(enc)
            if it >= 3:
                tf.append(a)
                te.append(b)
        rb = rb_t.cpu().numpy()
        assert [int(rb[f + 1] - rb[f]) for f in range(K)] == counts, "catch-up counts"
        assert int(foff[total].cpu()) == total * 86, "catch-up bytes"  # (every frame is 86 bytes again)
        res["catch_up"][f"K{K}"] = {"filters": K, "rows_out": total, "out_bytes": total * 86, "fanout_ms": _stat(tf),
                                    "encode_ms": _stat(te),
                                    "total_ms_median": statistics.median(tf) + statistics.median(te)}
        print("store catch-up", K, res["catch_up"][f"K{K}"], file=sys.stderr, flush=True)
        rows = foff = out = None
        torch.cuda.empty_cache()
    return res


# ---- merge report: the plain merge, the report's cost, the hub step ---------------------------------

NEWS_KS = (1, 8, 64)
NEWS_SHARES = (0, 10, 100)  # per cent of the hub batch's winners that are news to the store


def _news_timed(ctx, torch, dev):
    ext = ctx._ext(dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(ext)
        fn()
        e1.record(ext)
        e1.synchronize()
        return e0.elapsed_time(e1)
    return timed


def _merge_sequences(ctx, drp_amd, torch, wire_t, cols, m, keys, arena_bytes, seqs, merge):
    """The store leg's sequences (8 batches into an empty store, one warm-up sequence) under
    merge(store, view): [seq][batch] ms, and the last store's record."""
    timed = _news_timed(ctx, torch, torch.device("cuda", 0))
    out, store = [], None
    for it in range(seqs + 1):
        store = None
        torch.cuda.empty_cache()
        store = drp_amd.Store(ctx, keys, arena_bytes)
        tm = []
        for b in range(STORE_BATCHES):
            view = {k: v[b * m:] for k, v in cols.items()}
            tm.append(timed(lambda: merge(store, view)))
        if it:
            out.append(tm)
    return out, store.query().as_dict()


def _whole_batch_relay(ctx, drp_amd, torch, wire_t, view, m, iters):
    """Relaying the whole batch to K all-pass peers: drp_fanout_device and drp_encode_device over its m
    rows (what a hub without the report sends)."""
    dev = torch.device("cuda", 0)
    timed = _news_timed(ctx, torch, dev)
    res = {}
    for K in NEWS_KS:
        total = K * m
        rows = _row_tensors(torch, dev, total)
        rb_t = torch.zeros(K + 1, dtype=torch.int64, device=dev)
        foff = torch.zeros(total + 1, dtype=torch.int64, device=dev)
        out = torch.zeros(total * 86, dtype=torch.uint8, device=dev)
        flt = [None] * K
        tf, te = [], []
        for it in range(iters + 2):
            a = timed(lambda: ctx.fanout_device(wire_t, view, m, flt, rows, total, None, rb_t))
            b = timed(lambda: ctx.encode_device(rows, wire_t, total, foff, out, out.numel()))
            if it >= 2:
                tf.append(a)
                te.append(b)
        assert int(rb_t.cpu()[K]) == total and int(foff[total].cpu()) == total * 86
        res[f"K{K}"] = {"filters": K, "rows_out": total, "out_bytes": total * 86, "fanout_ms": _stat(tf),
                        "encode_ms": _stat(te), "total_ms_median": statistics.median(tf) + statistics.median(te)}
        print("whole-batch relay", K, res[f"K{K}"], file=sys.stderr, flush=True)
        rows = foff = out = None
        torch.cuda.empty_cache()
    return res


def news_baseline(ctx, drp_amd, torch, frames, seqs, iters):
    """What the parent commit's library can take: the plain merge sequences and the whole-batch relay."""
    key_ids, wire_t, cols, n, m = _store_input(ctx, drp_amd, torch, frames)
    keys = int(len(np.unique(key_ids)))
    arena_bytes = 80 * (keys + STORE_BATCHES * m) // 2
    merges, info = _merge_sequences(ctx, drp_amd, torch, wire_t, cols, m, keys, arena_bytes, seqs,
                                    lambda s, v: ctx.store_merge_device(s, wire_t, v, m))
    return {"bench": "relay_news_baseline", "frames": n, "batch_rows": m, "seqs": seqs, "merge_ms": _per_batch(merges),
            "final_info": info, "whole_batch": _whole_batch_relay(ctx, drp_amd, torch, wire_t, cols, m, iters)}


def news_leg(ctx, drp_amd, torch, frames, seqs, iters, parent=None):
    dev = torch.device("cuda", 0)
    key_ids, wire_t, cols, n, m = _store_input(ctx, drp_amd, torch, frames)
    keys = int(len(np.unique(key_ids)))
    arena_bytes = 80 * (keys + STORE_BATCHES * m) // 2
    timed = _news_timed(ctx, torch, dev)
    z = lambda k, dt: torch.zeros(max(k, 1), dtype=dt, device=dev)
    outcome, news, reply, ridx, nrep = z(m, torch.uint8), z(m, torch.uint8), _row_tensors(torch, dev, m), z(m, torch.int64), \
        z(1, torch.int64)
    legs = {"merge_ms": lambda s, v: ctx.store_merge_device(s, wire_t, v, m),
            "null_report_ms": lambda s, v: ctx.store_merge_report_device(s, wire_t, v, m, report=False),
            "full_report_ms": lambda s, v: ctx.store_merge_report_device(s, wire_t, v, m, None, outcome, news, reply, ridx,
                                                                         nrep, m, drp_amd.REPORT_KEEP_BLOBS)}
    res = {"frames": n, "batches": STORE_BATCHES, "batch_rows": m, "keys": keys, "seqs": seqs}
    infos = {}
    for name, fn in legs.items():
        ts, infos[name] = _merge_sequences(ctx, drp_amd, torch, wire_t, cols, m, keys, arena_bytes, seqs, fn)
        res[name] = _per_batch(ts)
        res["sum_" + name] = sum(x["median"] for x in res[name])
        print("news", name, res["sum_" + name], file=sys.stderr, flush=True)
    assert infos["merge_ms"] == infos["null_report_ms"] == infos["full_report_ms"], "the three merges' stores"
    res["final_info"] = infos["merge_ms"]
    res["full_over_merge"] = res["sum_full_report_ms"] / res["sum_merge_ms"]
    if parent is not None:
        assert parent["frames"] == n and parent["batch_rows"] == m and parent["final_info"] == res["final_info"]
        res["parent_merge_ms"] = parent["merge_ms"]
        res["sum_parent_merge_ms"] = sum(x["median"] for x in parent["merge_ms"])
        # (a): this build's median inside the parent's own min-max spread, batch by batch
        for name in ("merge_ms", "null_report_ms"):
            res[name + "_in_parent_spread"] = [p["min"] <= x["median"] <= p["max"]
                                               for x, p in zip(res[name], parent["merge_ms"])]
            res[name + "_over_parent"] = [x["median"] / p["median"] for x, p in zip(res[name], parent["merge_ms"])]
    # (c) the hub step over batch 0: merge with the news column, fan-out over the news view, encode
    view = cols
    raised = torch.from_numpy(np.where(np.asarray(key_ids[:m]) % 10 == 0, 1000, 0).astype(np.int64)).to(dev)
    bumped = {**view, "change": view["change"][:m] + raised}  # (every row of every tenth key: its winner is replaced)
    res["whole_batch"] = _whole_batch_relay(ctx, drp_amd, torch, wire_t, view, m, iters)
    if parent is not None:
        res["parent_whole_batch"] = parent["whole_batch"]
    res["hub"] = {}
    for share in NEWS_SHARES:
        batch = bumped if share == 10 else view
        for K in NEWS_KS:
            total = K * m
            rows = _row_tensors(torch, dev, total)
            rb_t = torch.zeros(K + 1, dtype=torch.int64, device=dev)
            foff = torch.zeros(total + 1, dtype=torch.int64, device=dev)
            out = torch.zeros(total * 86, dtype=torch.uint8, device=dev)
            flt = [None] * K
            tm, tf, te, sent, info = [], [], [], 0, None
            for it in range(iters + 2):
                store = drp_amd.Store(ctx, keys, arena_bytes)
                if share != 100:  # (the store holds the batch already; at 10: all but the raised changes)
                    ctx.store_merge_device(store, wire_t, view, m)
                a = timed(lambda: ctx.store_merge_report_device(store, wire_t, batch, m, None, None, news,
                                                                flags=drp_amd.REPORT_KEEP_BLOBS))
                b = timed(lambda: ctx.fanout_device(wire_t, {**batch, "type": news}, m, flt, rows, total, None, rb_t))
                sent = int(rb_t.cpu()[K])
                c = timed(lambda: ctx.encode_device(rows, wire_t, sent, foff, out, out.numel())) if sent else 0.0
                info = store.query()
                if it >= 2:
                    tm.append(a)
                    tf.append(b)
                    te.append(c)
            assert sent == K * (info.inserted + info.replaced) and info.refused == 0
            out_bytes = int(foff[sent].cpu()) if sent else 0
            whole = res["whole_batch"][f"K{K}"]
            r = {"filters": K, "news_rows": sent // K, "winners": int(info.winners), "rows_out": sent, "out_bytes": out_bytes,
                 "merge_report_ms": _stat(tm), "fanout_ms": _stat(tf), "encode_ms": _stat(te),
                 "total_ms_median": statistics.median(tm) + statistics.median(tf) + statistics.median(te),
                 "whole_batch_total_ms_median": whole["total_ms_median"], "whole_batch_out_bytes": whole["out_bytes"]}
            res["hub"][f"news{share}_K{K}"] = r
            print("hub step", share, K, r, file=sys.stderr, flush=True)
            rows = foff = out = None
            torch.cuda.empty_cache()
    return res


# ---- ordered catch-up -----------------------------------------------------------------------------

ORDER_KS = (1, 8, 64)
ORDER_LIMIT = 1000


def _final_store(ctx, drp_amd, torch, frames):
    """The store leg's final store: the keyed stream merged as 8 batches into an empty store, compacted."""
    dev = torch.device("cuda", 0)
    key_ids, wire_t, cols, n, m = _store_input(ctx, drp_amd, torch, frames)
    keys = int(len(np.unique(key_ids)))
    store = drp_amd.Store(ctx, keys, 80 * (keys + STORE_BATCHES * m) // 2)
    for b in range(STORE_BATCHES):
        ctx.store_merge_device(store, wire_t, {k: v[b * m:] for k, v in cols.items()}, m)
    before = store.query()
    assert before.rows == keys and before.refused == 0, (before.rows, keys)
    a2 = torch.zeros(before.arena_used, dtype=torch.uint8, device=dev)
    ctx.store_compact(store, a2)
    assert store.query().refused == 0
    store.arena, store.arena_bytes = a2, a2.numel()
    del wire_t, cols
    torch.cuda.empty_cache()
    return store, keys, n


def _order_shape(ctx, drp_amd, torch, store, ch, K, stat):
    """The catch-up shape K of the store leg: its filters, the fan-out's rows and bounds, and the
    timings of drp_fanout_device and of drp_encode_device over all rows (the yardstick)."""
    dev = torch.device("cuda", 0)
    ts_ = [(100 * f) // K for f in range(K)]
    flt = [drp_amd.make_filter(change_range=(t + 1, 2**64 - 1)) for t in ts_]
    counts = [int((ch > t).sum()) for t in ts_]
    total = sum(counts)
    rows = _row_tensors(torch, dev, total)
    rb_t = torch.zeros(K + 1, dtype=torch.int64, device=dev)
    foff = torch.zeros(total + 1, dtype=torch.int64, device=dev)
    out = torch.zeros(total * 86, dtype=torch.uint8, device=dev)
    tf = stat(lambda: ctx.fanout_device(store.arena, store.cols, store.max_keys, flt, rows, total, None, rb_t))
    te = stat(lambda: ctx.encode_device(rows, store.arena, total, foff, out, out.numel()))
    rb = rb_t.cpu().numpy()
    assert [int(rb[f + 1] - rb[f]) for f in range(K)] == counts, "catch-up counts"
    assert int(foff[total].cpu()) == total * 86, "catch-up bytes"
    res = {"filters": K, "rows_out": total, "fanout_ms": tf, "encode_ms": te}
    return res, rows, rb_t, rb, foff, out


def order_baseline(ctx, drp_amd, torch, frames, iters):
    """The yardstick alone (no call of this commit): the parent's library and binding can take it."""
    store, keys, n = _final_store(ctx, drp_amd, torch, frames)
    ch = store.cols["change"][:keys].cpu().numpy()
    stat = _timers(ctx, torch, torch.device("cuda", 0), iters)
    res = {"bench": "relay_order_baseline", "frames": n, "keys": keys, "iters": iters}
    for K in ORDER_KS:
        res[f"K{K}"] = _order_shape(ctx, drp_amd, torch, store, ch, K, stat)[0]
        print("order baseline", K, res[f"K{K}"], file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    return res


def _order_expect(chg, rb, limit=None):
    """numpy: per segment the stable argsort of the keys (unsigned), cut to `limit` rows."""
    perm, ob = [], [0]
    for f in range(len(rb) - 1):
        lo, hi = int(rb[f]), int(rb[f + 1])
        o = lo + np.argsort(chg[lo:hi], kind="stable")
        if limit is not None:
            o = o[:limit]
        perm.append(o)
        ob.append(ob[-1] + len(o))
    return np.concatenate(perm), ob


def order_leg(ctx, drp_amd, torch, frames, iters, parent=None, profile=False):
    dev = torch.device("cuda", 0)
    store, keys, n = _final_store(ctx, drp_amd, torch, frames)
    ch = store.cols["change"][:keys].cpu().numpy()
    stat = _timers(ctx, torch, dev, iters)
    if profile:  # (for a kernel trace: K = 64 and the plain call alone, so that a kernel's total is per call)
        K = ORDER_KS[-1]
        r, rows, rb_t, rb, foff, out = _order_shape(ctx, drp_amd, torch, store, ch, K, stat)
        out_rows = _row_tensors(torch, dev, r["rows_out"])
        ob_t = torch.zeros(K + 1, dtype=torch.int64, device=dev)
        r["order_ms"] = stat(lambda: ctx.order_device(rows, rb_t, K, r["rows_out"], out_rows, ob_t))
        r["order_calls"] = iters + 3
        return {"frames": n, "keys": keys, "iters": iters, f"K{K}": r}
    os.environ["DRP_ORDER_SKIP"] = "0"  # (read when a ctx opens: ctx2 runs every pass)
    ctx2 = drp_amd.Ctx(0)
    del os.environ["DRP_ORDER_SKIP"]
    stat2 = _timers(ctx2, torch, dev, iters)
    res = {"frames": n, "keys": keys, "iters": iters, "limit": ORDER_LIMIT}
    for K in ORDER_KS:
        r, rows, rb_t, rb, foff, out = _order_shape(ctx, drp_amd, torch, store, ch, K, stat)
        total = r["rows_out"]
        out_rows = _row_tensors(torch, dev, total)
        ob_t = torch.zeros(K + 1, dtype=torch.int64, device=dev)
        sel = torch.arange(total, dtype=torch.int64, device=dev)
        osel = torch.zeros(total, dtype=torch.int64, device=dev)

        def checked(c, src, limit=None):
            """One call with sel_idx = arange against numpy: the permutation, the keys, out_base."""
            c.order_device(src, rb_t, K, total, out_rows, ob_t, limit=limit, sel_idx_t=sel, out_sel_idx_t=osel)
            torch.cuda.synchronize()
            chg = src["change"].cpu().numpy().view(np.uint64)
            perm, ob = _order_expect(chg, rb, limit)
            assert [int(v) for v in ob_t.cpu()] == ob, "order out_base"
            assert np.array_equal(osel[:ob[-1]].cpu().numpy(), perm), "order permutation"
            assert np.array_equal(out_rows["change"][:ob[-1]].cpu().numpy().view(np.uint64), chg[perm]), "order keys"
            return ob[-1]

        checked(ctx, rows)
        r["order_ms"] = stat(lambda: ctx.order_device(rows, rb_t, K, total, out_rows, ob_t))
        checked(ctx2, rows)
        r["order_every_pass_ms"] = stat2(lambda: ctx2.order_device(rows, rb_t, K, total, out_rows, ob_t))
        sent = checked(ctx, rows, ORDER_LIMIT)
        r["order_limit_ms"] = stat(lambda: ctx.order_device(rows, rb_t, K, total, out_rows, ob_t, limit=ORDER_LIMIT))
        r["page_rows"] = sent
        r["encode_page_ms"] = stat(lambda: ctx.encode_device(out_rows, store.arena, sent, foff, out, out.numel()))
        assert int(foff[sent].cpu()) == sent * 86, "page bytes"
        # uniform 64-bit keys in the same rows and segments
        r32 = lambda: torch.randint(0, 2**32, (total,), dtype=torch.int64, device=dev)
        uni = dict(rows, change=(r32() << 32) | r32())
        checked(ctx, uni)
        r["uniform_order_ms"] = stat(lambda: ctx.order_device(uni, rb_t, K, total, out_rows, ob_t))
        checked(ctx2, uni)
        r["uniform_order_every_pass_ms"] = stat2(lambda: ctx2.order_device(uni, rb_t, K, total, out_rows, ob_t))
        r["order_over_encode"] = r["order_ms"]["median"] / r["encode_ms"]["median"]
        if parent is not None:
            p = parent[f"K{K}"]
            assert p["rows_out"] == total
            r["parent_fanout_ms"], r["parent_encode_ms"] = p["fanout_ms"], p["encode_ms"]
            r["order_over_parent_encode"] = r["order_ms"]["median"] / p["encode_ms"]["median"]
        res[f"K{K}"] = r
        print("order", K, r, file=sys.stderr, flush=True)
        rows = out_rows = uni = foff = out = sel = osel = None
        torch.cuda.empty_cache()
    ctx2.close()
    return res


# ---- key-ordered listing ----------------------------------------------------------------------------

KEYORDER_KS = (1, 64)
KEYORDER_PREFIX = b"tenant-00000001/"


def _keyorder_chain(mat, lens, K):
    """The launcher's rule applied to the keys (mat: rows x longest, zero padded; no subsets): the
    fields launched, the digit passes that run in them (those in which two values differ), kernels."""
    longest = int(lens.max())
    fields, active, launches = 0, 0, 3 + 2 + (5 if K > 1 else 0)

    def field(vals, p_lo, p_hi):
        nonlocal fields, active, launches
        diff = int(np.bitwise_or.reduce(vals)) ^ int(np.bitwise_and.reduce(vals))
        fields += 1
        active += sum(1 for p in range(p_lo, p_hi) if (diff >> (8 * p)) & 0xFF)
        launches += 2 + 4 * (p_hi - p_lo)

    field(lens.astype(np.uint64), 0, 2)
    nw = (longest + 7) // 8
    pad = np.zeros((mat.shape[0], nw * 8), np.uint8)
    pad[:, :longest] = mat
    words = pad.reshape(-1, nw, 8).view(">u8")[:, :, 0].astype(np.uint64)
    shared = 0  # leading words that lie whole inside every key and are the same in all: not launched
    while shared < int(lens.min()) // 8 and (words[:, shared] == words[0, shared]).all():
        shared += 1
    for w in range(nw - 1, shared - 1, -1):
        field(words[:, w], 8 - longest % 8 if w == nw - 1 and longest % 8 else 0, 8)
    return {"fields": fields, "shared_prefix_words": shared, "active_digit_passes": active + (1 if K > 1 else 0), "launches": launches, "host_waits": 1}


def keyorder_leg(ctx, drp_amd, torch, frames, iters):
    import time
    dev = torch.device("cuda", 0)
    store, keys, n = _final_store(ctx, drp_amd, torch, frames)
    ch = store.cols["change"][:keys].cpu().numpy()
    stat = _timers(ctx, torch, dev, iters)
    os.environ["DRP_ORDER_SKIP"] = "0"  # (read when a ctx opens: ctx2 runs every pass)
    ctx2 = drp_amd.Ctx(0)
    del os.environ["DRP_ORDER_SKIP"]
    stat2 = _timers(ctx2, torch, dev, iters)
    res = {"frames": n, "keys": keys, "iters": iters}
    for K in KEYORDER_KS:
        # K version-bounded listings that share the store's rows out among them (change is 1 .. 100)
        edge = [0] + [(100 * (f + 1)) // K + 1 for f in range(K - 1)] + [2**64]
        flt = [drp_amd.make_filter(change_range=(edge[f], edge[f + 1] - 1)) for f in range(K)]
        total = keys
        rows = _row_tensors(torch, dev, total)
        rb_t = torch.zeros(K + 1, dtype=torch.int64, device=dev)
        ctx.fanout_device(store.arena, store.cols, store.max_keys, flt, rows, total, None, rb_t)
        torch.cuda.synchronize()
        rb = rb_t.cpu().numpy()
        assert int(rb[K]) == total and not bool((rows["flags"] & 1).any())
        out_rows = _row_tensors(torch, dev, total)
        ob_t = torch.zeros(K + 1, dtype=torch.int64, device=dev)
        osel = torch.zeros(total, dtype=torch.int64, device=dev)
        tot_t = torch.zeros(2, dtype=torch.int64, device=dev)
        none = [drp_amd.make_key_page(limit=0)] * K
        r = {"filters": K, "rows": total}
        r["order_every_pass_ms"] = stat2(lambda: ctx2.order_device(rows, rb_t, K, total, out_rows, ob_t))
        r["order_every_pass_digit_passes"] = 8 + (1 if K > 1 else 0)
        # the keys on the host: the copy and the sort a peer would do today
        t0 = time.perf_counter()
        arena = store.arena.cpu().numpy()
        koff, klen = rows["key_off"].cpu().numpy(), rows["key_len"].cpu().numpy()
        t1 = time.perf_counter()
        longest = int(klen.max())
        mat = arena[np.minimum(koff[:, None] + np.arange(longest), len(arena) - 1)]
        mat[np.arange(longest)[None, :] >= klen[:, None]] = 0
        t2 = time.perf_counter()
        assert not (mat == 0).any(), "numpy's S compare needs keys without NUL bytes"
        fixed = np.ascontiguousarray(mat).view("S%d" % longest)[:, 0]
        perm = [int(rb[f]) + np.argsort(fixed[int(rb[f]):int(rb[f + 1])], kind="stable") for f in range(K)]
        t3 = time.perf_counter()
        r["host_numpy"] = {"copy_ms": (t1 - t0) * 1e3, "gather_keys_ms": (t2 - t1) * 1e3, "argsort_ms": (t3 - t2) * 1e3,
                           "total_ms": (t3 - t0) * 1e3}
        for name in ("own_keys", "prefix16"):
            if name == "own_keys":
                heap, src, m = store.arena, rows, mat
            else:  # the same keys behind a shared prefix, in a heap of their own
                m = np.concatenate([np.tile(np.frombuffer(KEYORDER_PREFIX, np.uint8), (total, 1)), mat], axis=1)
                lens2 = klen.astype(np.int64) + 16
                heap = torch.from_numpy(m[np.arange(m.shape[1])[None, :] < lens2[:, None]]).to(dev)
                off2 = torch.from_numpy(np.concatenate([[0], np.cumsum(lens2)[:-1]])).to(dev)
                src = dict(rows, key_off=off2, key_len=rows["key_len"] + 16)
            lens = klen.astype(np.int64) + (0 if name == "own_keys" else 16)
            w = _keyorder_chain(m, lens, K)
            ctx.order_keys_device(heap, src, rb_t, K, total, out_rows, ob_t, sel_idx_t=torch.arange(total, device=dev),
                                  out_sel_idx_t=osel, totals_t=tot_t)
            torch.cuda.synchronize()
            assert [int(v) for v in tot_t.cpu()] == [total, 0] and [int(v) for v in ob_t.cpu()] == [int(v - rb[0]) for v in rb]
            assert np.array_equal(osel.cpu().numpy(), np.concatenate(perm)), "key order permutation"
            w["call_ms"] = stat(lambda: ctx.order_keys_device(heap, src, rb_t, K, total, out_rows, ob_t))
            w["sort_ms"] = stat(lambda: ctx.order_keys_device(heap, src, rb_t, K, total, out_rows, ob_t, pages=none))
            w["sort_ms_per_active_pass"] = w["sort_ms"]["median"] / max(1, w["active_digit_passes"])
            w["order_every_pass_ms_per_pass"] = r["order_every_pass_ms"]["median"] / r["order_every_pass_digit_passes"]
            w["host_over_device"] = r["host_numpy"]["total_ms"] / w["call_ms"]["median"]
            r[name] = w
        res[f"K{K}"] = r
        print("keyorder", K, r, file=sys.stderr, flush=True)
        rows = out_rows = osel = src = heap = mat = m = None
        torch.cuda.empty_cache()
    ctx2.close()
    return res


# ---- digest / reconcile -----------------------------------------------------------------------------

DIGEST_BITS = (8, 12, 16)
RECONCILE_BITS = 16
BIG_KEYS, BIG_VALUE = 65536, 4096


def big_value_stream(n, vlen=BIG_VALUE, seed=3):
    """n Changes with the 10-digit keys 0 .. n - 1 and vlen random value bytes (two-byte varints:
    128 <= vlen < 16000): change = i % 100 + 1, from = i % 128, to = (i + 1) % 128; 24 + vlen bytes a frame."""
    plen = 21 + vlen
    assert 128 <= vlen and plen + 1 < 16384
    i = np.arange(n, dtype=np.int64)
    a = np.zeros((n, plen + 3), np.uint8)
    a[:, 0], a[:, 1], a[:, 2] = ((plen + 1) & 0x7F) | 0x80, (plen + 1) >> 7, 1
    a[:, 3], a[:, 4] = 0x12, 10
    for k in range(10):
        a[:, 5 + k] = 48 + (i // 10 ** (9 - k)) % 10
    a[:, 15], a[:, 16] = 0x18, (i % 100) + 1
    a[:, 17], a[:, 18] = 0x20, i % 128
    a[:, 19], a[:, 20] = 0x28, (i + 1) % 128
    a[:, 21], a[:, 22], a[:, 23] = 0x32, (vlen & 0x7F) | 0x80, vlen >> 7
    a[:, 24:] = np.random.default_rng(seed).integers(0, 256, size=(n, vlen), dtype=np.uint8)
    return a.reshape(-1)


def _digest_store(ctx, drp_amd, torch, shape, frames):
    """One of the leg's two stores, compacted: (store, keys, frame bytes of a stored row re-encoded).
    "keyed": the store leg's final store (frames keyed C2 rows in 8 merges); "big_values": BIG_KEYS keys
    with BIG_VALUE-byte values in one merge. Only calls every commit with a store has."""
    dev = torch.device("cuda", 0)
    if shape == "keyed":
        key_ids, wire_t, cols, n, m = _store_input(ctx, drp_amd, torch, frames)
        keys, batches, fb = int(len(np.unique(key_ids))), STORE_BATCHES, 86
        arena_bytes = 80 * (keys + STORE_BATCHES * m) // 2
    else:
        wire_t, cols, n = device_setup(ctx, drp_amd, torch, None, BIG_KEYS, wire=big_value_stream(BIG_KEYS))
        keys, batches, m, fb = BIG_KEYS, 1, BIG_KEYS, 24 + BIG_VALUE
        arena_bytes = keys * ((10 + BIG_VALUE + 15) & ~15)
    store = drp_amd.Store(ctx, keys, arena_bytes)
    for b in range(batches):
        ctx.store_merge_device(store, wire_t, {k: v[b * m:] for k, v in cols.items()}, m)
    info = store.query()
    assert info.refused == 0 and info.rows == keys, (info.rows, keys, info.refused)
    a2 = torch.zeros(info.arena_used - info.arena_dead, dtype=torch.uint8, device=dev)
    ctx.store_compact(store, a2)
    assert store.query().refused == 0
    store.arena, store.arena_bytes = a2, a2.numel()
    del wire_t, cols
    torch.cuda.empty_cache()
    return store, keys, fb


def _digest_yardsticks(ctx, drp_amd, torch, store, keys, fb, iters):
    """The two existing passes the digest is set against: drp_store_compact of the store (between two
    arenas, to and fro) and the full snapshot a hub sends today (drp_fanout_device with one all-pass
    filter over the store's view and drp_encode_device). HIP events; three warm-up rounds."""
    dev = torch.device("cuda", 0)
    ext = ctx._ext(dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(ext)
        fn()
        e1.record(ext)
        e1.synchronize()
        return e0.elapsed_time(e1)

    live = store.arena_bytes
    spare = torch.zeros(live, dtype=torch.uint8, device=dev)
    rows = _row_tensors(torch, dev, keys)
    rb_t = torch.zeros(2, dtype=torch.int64, device=dev)
    foff = torch.zeros(keys + 1, dtype=torch.int64, device=dev)
    out = torch.zeros(keys * fb, dtype=torch.uint8, device=dev)
    flt = [None]
    tc, tf, te = [], [], []
    for it in range(iters + 3):
        a2 = spare
        c = timed(lambda: ctx.store_compact(store, a2))
        assert store.query().refused == 0
        spare, store.arena = store.arena, a2
        f = timed(lambda: ctx.fanout_device(store.arena, store.cols, store.max_keys, flt, rows, keys, None, rb_t))
        e = timed(lambda: ctx.encode_device(rows, store.arena, keys, foff, out, out.numel()))
        if it >= 3:
            tc.append(c)
            tf.append(f)
            te.append(e)
    assert int(rb_t.cpu()[1]) == keys and int(foff[keys].cpu()) == keys * fb, "snapshot"
    return {"keys": keys, "live_bytes": live, "compact_ms": _stat(tc),
            "snapshot": {"rows_out": keys, "out_bytes": keys * fb, "fanout_ms": _stat(tf), "encode_ms": _stat(te),
                         "total_ms_median": statistics.median(tf) + statistics.median(te)}}


def digest_baseline(ctx, drp_amd, torch, frames, iters):
    res = {"bench": "relay_digest_baseline", "frames": frames, "iters": iters}
    for shape in ("keyed", "big_values"):
        store, keys, fb = _digest_store(ctx, drp_amd, torch, shape, frames)
        res[shape] = _digest_yardsticks(ctx, drp_amd, torch, store, keys, fb, iters)
        print("digest baseline", shape, res[shape], file=sys.stderr, flush=True)
        store = None
        torch.cuda.empty_cache()
    return res


def digest_leg(ctx, drp_amd, torch, frames, iters, parent=None):
    dev = torch.device("cuda", 0)
    ext = ctx._ext(dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(ext)
        fn()
        e1.record(ext)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def runs(fn):
        return _stat([timed(fn) for it in range(iters + 3)][3:])

    res = {"frames": frames, "iters": iters}
    for shape in ("keyed", "big_values"):
        store, keys, fb = _digest_store(ctx, drp_amd, torch, shape, frames)
        r = _digest_yardsticks(ctx, drp_amd, torch, store, keys, fb, iters)
        view, n = store.arena, store.max_keys
        tot = torch.zeros(2, dtype=torch.int64, device=dev)
        r["digest_ms"], mine = {}, {}
        for bits in DIGEST_BITS:
            cells = torch.zeros((1 << bits, 2), dtype=torch.int64, device=dev)
            r["digest_ms"][f"bits{bits}"] = runs(lambda: ctx.digest_device(view, store.cols, n, None, bits, cells, tot))
            assert [int(v) for v in tot.cpu()] == [keys, 0] and int(cells[:, 0].sum().cpu()) == keys, "digest totals"
            mine[bits] = cells
        base = (parent or {}).get(shape, r)
        r["yardsticks_from"] = "parent" if parent else "this commit"
        r["parent"] = base if parent else None
        r["digest_over_compact"] = {k: v["median"] / base["compact_ms"]["median"] for k, v in r["digest_ms"].items()}
        # the peer: the same rows with `change` raised on a random share of the keys
        bits = RECONCILE_BITS
        words = (1 << bits) // 64
        bset = torch.zeros(words, dtype=torch.int64, device=dev)
        cnt = torch.zeros(2, dtype=torch.int64, device=dev)
        rows = _row_tensors(torch, dev, keys)
        idx_t = torch.zeros(keys, dtype=torch.int64, device=dev)
        foff = torch.zeros(keys + 1, dtype=torch.int64, device=dev)
        out = torch.zeros(keys * fb, dtype=torch.uint8, device=dev)
        r["reconcile"] = {}
        for share in (0.001, 0.10):
            gen = torch.Generator(device="cpu").manual_seed(int(share * 1000))
            hit = torch.randperm(keys, generator=gen)[:max(1, int(keys * share))].to(dev)
            peer_cols = dict(store.cols)
            peer_cols["change"] = store.cols["change"].clone()
            peer_cols["change"][hit] += 1
            peer = torch.zeros((1 << bits, 2), dtype=torch.int64, device=dev)
            ctx.digest_device(view, peer_cols, n, None, bits, peer, None)
            t_diff = runs(lambda: ctx.digest_diff_device(mine[bits], peer, bits, bset, cnt[0:1]))
            t_sel = runs(lambda: ctx.select_buckets_device(view, store.cols, n, None, bits, bset, rows, idx_t, cnt[1:2]))
            nd, nsel = [int(v) for v in cnt.cpu()]
            got = torch.zeros(keys, dtype=torch.bool, device=dev)
            got[idx_t[:nsel]] = True
            assert bool(got[hit].all()) and len(hit) >= nd > 0 and nsel >= len(hit), "reconcile rows"
            # (cap = the bytes needed, as Store.reconcile passes it: the encoder's write grid is sized from cap)
            t_enc = runs(lambda: ctx.encode_device(rows, view, nsel, foff, out, nsel * fb))
            assert int(foff[nsel].cpu()) == nsel * fb, "reconcile bytes"
            total = (r["digest_ms"][f"bits{bits}"]["median"] + t_diff["median"] + t_sel["median"] + t_enc["median"])
            r["reconcile"][f"share{share}"] = {
                "bits": bits, "keys_altered": int(len(hit)), "buckets_differing": nd, "rows_out": nsel,
                "out_bytes": nsel * fb, "cells_bytes": 16 << bits, "diff_ms": t_diff, "select_buckets_ms": t_sel,
                "encode_ms": t_enc, "total_ms_median": total,
                "over_snapshot": total / base["snapshot"]["total_ms_median"],
                "bytes_over_snapshot": (nsel * fb + (16 << bits)) / base["snapshot"]["out_bytes"]}
            print("digest reconcile", shape, share, r["reconcile"][f"share{share}"], file=sys.stderr, flush=True)
        res[shape] = r
        print("digest", shape, r["digest_ms"], r["compact_ms"], r["digest_over_compact"], file=sys.stderr, flush=True)
        store = view = rows = out = mine = None
        torch.cuda.empty_cache()
    return res


# ---- refined digests --------------------------------------------------------------------------------

REFINE_SUB_BITS = (2, 4, 8)
REFINE_SHARES = (0.001, 0.10)


def _timers(ctx, torch, dev, iters):
    ext = ctx._ext(dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(ext)
        fn()
        e1.record(ext)
        e1.synchronize()
        return e0.elapsed_time(e1)

    return lambda fn: _stat([timed(fn) for it in range(iters + 3)][3:])


def _peer_cols(torch, store, keys, share, dev):
    """The digest leg's peer: the same rows with `change` raised on a random share of the keys."""
    gen = torch.Generator(device="cpu").manual_seed(int(share * 1000))
    hit = torch.randperm(keys, generator=gen)[:max(1, int(keys * share))].to(dev)
    cols = dict(store.cols)
    cols["change"] = store.cols["change"].clone()
    cols["change"][hit] += 1
    return cols, hit


def _single_level(ctx, torch, store, keys, fb, iters):
    """The single-level reconcile at RECONCILE_BITS per altered share, through calls every commit with
    the digest has: digest, diff, bucket select, encode."""
    dev = torch.device("cuda", 0)
    runs = _timers(ctx, torch, dev, iters)
    view, n, bits = store.arena, store.max_keys, RECONCILE_BITS
    mine = torch.zeros((1 << bits, 2), dtype=torch.int64, device=dev)
    t_dig = runs(lambda: ctx.digest_device(view, store.cols, n, None, bits, mine, None))
    bset = torch.zeros((1 << bits) // 64, dtype=torch.int64, device=dev)
    cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    rows = _row_tensors(torch, dev, keys)
    foff = torch.zeros(keys + 1, dtype=torch.int64, device=dev)
    out = torch.zeros(keys * fb, dtype=torch.uint8, device=dev)
    res = {"digest_ms": t_dig}
    for share in REFINE_SHARES:
        peer_cols, hit = _peer_cols(torch, store, keys, share, dev)
        peer = torch.zeros((1 << bits, 2), dtype=torch.int64, device=dev)
        ctx.digest_device(view, peer_cols, n, None, bits, peer, None)
        t_diff = runs(lambda: ctx.digest_diff_device(mine, peer, bits, bset, cnt[0:1]))
        t_sel = runs(lambda: ctx.select_buckets_device(view, store.cols, n, None, bits, bset, rows, None, cnt[1:2]))
        nd, nsel = [int(v) for v in cnt.cpu()]
        t_enc = runs(lambda: ctx.encode_device(rows, view, nsel, foff, out, nsel * fb))
        res[f"share{share}"] = {
            "keys_altered": int(len(hit)), "buckets_differing": nd, "rows_out": nsel, "diff_ms": t_diff,
            "select_buckets_ms": t_sel, "encode_ms": t_enc,
            "total_ms_median": t_dig["median"] + t_diff["median"] + t_sel["median"] + t_enc["median"],
            "bytes": {"cells": 16 << bits, "frames": nsel * fb, "total": (16 << bits) + nsel * fb}}
    return res


def digest_refine_baseline(ctx, drp_amd, torch, frames, iters):
    res = {"bench": "relay_digest_refine_baseline", "frames": frames, "iters": iters}
    for shape in ("keyed", "big_values"):
        store, keys, fb = _digest_store(ctx, drp_amd, torch, shape, frames)
        res[shape] = _digest_yardsticks(ctx, drp_amd, torch, store, keys, fb, iters)
        res[shape]["single_level"] = _single_level(ctx, torch, store, keys, fb, iters)
        print("digest refine baseline", shape, res[shape], file=sys.stderr, flush=True)
        store = None
        torch.cuda.empty_cache()
    return res


def digest_refine_leg(ctx, drp_amd, torch, frames, iters, parent=None):
    """Per store and altered share: the single-level reconcile of this build, and per sub_bits the
    refine, the cell diff, the refined select and the encode, the rows out and the bytes one hub sends
    (first-level cells, cells2, frames). Ratios are over the parent's figures where given."""
    dev = torch.device("cuda", 0)
    runs = _timers(ctx, torch, dev, iters)
    res = {"frames": frames, "iters": iters, "yardsticks_from": "parent" if parent else "this commit"}
    for shape in ("keyed", "big_values"):
        store, keys, fb = _digest_store(ctx, drp_amd, torch, shape, frames)
        r = _digest_yardsticks(ctx, drp_amd, torch, store, keys, fb, iters)
        r["single_level"] = _single_level(ctx, torch, store, keys, fb, iters)
        base = (parent or {}).get(shape, r)
        r["parent"] = base if parent else None
        view, n, bits = store.arena, store.max_keys, RECONCILE_BITS
        mine = torch.zeros((1 << bits, 2), dtype=torch.int64, device=dev)
        ctx.digest_device(view, store.cols, n, None, bits, mine, None)
        bset = torch.zeros((1 << bits) // 64, dtype=torch.int64, device=dev)
        cnt = torch.zeros(3, dtype=torch.int64, device=dev)
        tot = torch.zeros(3, dtype=torch.int64, device=dev)
        rows = _row_tensors(torch, dev, keys)
        idx_t = torch.zeros(keys, dtype=torch.int64, device=dev)
        foff = torch.zeros(keys + 1, dtype=torch.int64, device=dev)
        out = torch.zeros(keys * fb, dtype=torch.uint8, device=dev)
        r["refined"] = {}
        for share in REFINE_SHARES:
            peer_cols, hit = _peer_cols(torch, store, keys, share, dev)
            peer = torch.zeros((1 << bits, 2), dtype=torch.int64, device=dev)
            ctx.digest_device(view, peer_cols, n, None, bits, peer, None)
            ctx.digest_diff_device(mine, peer, bits, bset, cnt[0:1])
            nd = int(cnt.cpu()[0])
            one = base["single_level"][f"share{share}"]
            per = {}
            for sub_bits in REFINE_SUB_BITS:
                ncells = nd << sub_bits
                c_mine = torch.zeros((ncells, 2), dtype=torch.int64, device=dev)
                c_peer = torch.zeros((ncells, 2), dtype=torch.int64, device=dev)
                cset = torch.zeros((ncells + 63) // 64, dtype=torch.int64, device=dev)
                ctx.digest_refine_device(view, peer_cols, n, None, bits, bset, sub_bits, c_peer, ncells, tot)
                t_ref = runs(lambda: ctx.digest_refine_device(view, store.cols, n, None, bits, bset, sub_bits, c_mine,
                                                              ncells, tot))
                t = [int(v) for v in tot.cpu()]
                assert t[1] == 0 and t[2] == nd and t[0] == one["rows_out"], ("refine totals", t, nd, one["rows_out"])
                t_diff = runs(lambda: ctx.digest_diff_cells_device(c_mine, c_peer, ncells, cset, cnt[1:2]))
                t_sel = runs(lambda: ctx.select_refined_device(view, store.cols, n, None, bits, bset, sub_bits, cset, rows,
                                                               idx_t, cnt[2:3]))
                _, nd2, nsel = [int(v) for v in cnt.cpu()]
                got = torch.zeros(keys, dtype=torch.bool, device=dev)
                got[idx_t[:nsel]] = True
                assert bool(got[hit].all()) and len(hit) >= nd2 > 0 and one["rows_out"] >= nsel >= len(hit), "refined rows"
                t_enc = runs(lambda: ctx.encode_device(rows, view, nsel, foff, out, nsel * fb))
                assert int(foff[nsel].cpu()) == nsel * fb, "refined bytes"
                total = (base["single_level"]["digest_ms"]["median"] + one["diff_ms"]["median"] + t_ref["median"] +
                         t_diff["median"] + t_sel["median"] + t_enc["median"])
                nbytes = (16 << bits) + 16 * ncells + nsel * fb
                per[f"sub_bits{sub_bits}"] = {
                    "cells2": ncells, "cells_differing": nd2, "rows_out": nsel, "refine_ms": t_ref, "diff_cells_ms": t_diff,
                    "select_refined_ms": t_sel, "encode_ms": t_enc, "total_ms_median": total,
                    "bytes": {"cells": 16 << bits, "cells2": 16 * ncells, "frames": nsel * fb, "total": nbytes},
                    "over_single_level": total / one["total_ms_median"],
                    "over_snapshot": total / base["snapshot"]["total_ms_median"],
                    "bytes_over_single_level": nbytes / one["bytes"]["total"],
                    "bytes_over_snapshot": nbytes / base["snapshot"]["out_bytes"]}
                c_mine = c_peer = cset = None
            r["refined"][f"share{share}"] = {
                "keys_altered": int(len(hit)), "buckets_differing": nd,
                "single_level_bytes_over_snapshot": one["bytes"]["total"] / base["snapshot"]["out_bytes"],
                "single_level_over_snapshot": one["total_ms_median"] / base["snapshot"]["total_ms_median"], **per}
            print("digest refine", shape, share, r["refined"][f"share{share}"], file=sys.stderr, flush=True)
        # the LDS copy of the cells: every row a member, 256 and 1024 cells (summed in LDS) against 2048 and
        # 4096 (summed in global memory)
        r["lds_probe_ms"] = {}
        for b in (0, 2, 3, 4):
            full = torch.full((1,), (1 << (1 << b)) - 1, dtype=torch.int64, device=dev)
            c2 = torch.zeros((256 << b, 2), dtype=torch.int64, device=dev)
            r["lds_probe_ms"][f"cells{256 << b}"] = runs(
                lambda: ctx.digest_refine_device(view, store.cols, n, None, b, full, 8, c2, 256 << b, tot))
            assert [int(v) for v in tot.cpu()] == [keys, 0, 1 << b] and int(c2[:, 0].sum().cpu()) == keys
        print("digest refine lds probe", shape, r["lds_probe_ms"], file=sys.stderr, flush=True)
        res[shape] = r
        store = view = rows = out = mine = None
        torch.cuda.empty_cache()
    return res


# ---- lookup: point reads and the have-list against the store -----------------------------------------

LOOKUP_SIZES = (64, 65_536, 1_250_000)
LOOKUP_ABSENT_ID = 2_000_000_000  # (ten digits, above every key id of the stream)
HAVE_CHANGE = 50                  # the have-list's version: about half of the store lies above it


def _lookup_store(ctx, drp_amd, torch, frames, seqs):
    """The store leg's merge sequences, timed ([seq][batch] ms, one warm-up sequence), and its final
    store: the last sequence's, compacted. Through calls every commit with the store has."""
    dev = torch.device("cuda", 0)
    key_ids, wire_t, cols, n, m = _store_input(ctx, drp_amd, torch, frames)
    ids = np.unique(key_ids)
    keys = int(len(ids))
    timed = _news_timed(ctx, torch, dev)
    merges, store = [], None
    for it in range(seqs + 1):
        store = None
        torch.cuda.empty_cache()
        store = drp_amd.Store(ctx, keys, 80 * (keys + STORE_BATCHES * m) // 2)
        tm = [timed(lambda: ctx.store_merge_device(store, wire_t, {k: v[b * m:] for k, v in cols.items()}, m))
              for b in range(STORE_BATCHES)]
        if it:
            merges.append(tm)
    before = store.query()
    assert before.rows == keys and before.refused == 0, (before.rows, keys)
    a2 = torch.zeros(before.arena_used, dtype=torch.uint8, device=dev)
    ctx.store_compact(store, a2)
    assert store.query().refused == 0
    store.arena, store.arena_bytes = a2, a2.numel()
    del wire_t, cols
    torch.cuda.empty_cache()
    return store, ids, n, m, _per_batch(merges)


def _point_keys(ids, nq, seed=11):
    """nq key ids, half of them held (a seeded sample of the store's) and half not, shuffled."""
    rng = np.random.default_rng(seed)
    held = rng.choice(ids, nq // 2, replace=False)
    q = np.concatenate([held, LOOKUP_ABSENT_ID + np.arange(nq - nq // 2, dtype=np.int64)])
    rng.shuffle(q)
    return q, nq // 2


def _key_digits(q):
    a = np.zeros((len(q), 10), np.uint8)
    for k in range(10):
        a[:, k] = 48 + (q // 10 ** (9 - k)) % 10
    return a


def lookup_baseline(ctx, drp_amd, torch, frames, seqs, iters):
    """What the parent commit can do for a point read: one drp_fanout_device over the store with 64
    DRP_SEL_KEY_PREFIX filters (the 64-key lookup's keys, whole: a prefix of ten digits is the key) and
    the encode of the rows found; and the merge sequences. No call of this commit."""
    dev = torch.device("cuda", 0)
    store, ids, n, m, merge_ms = _lookup_store(ctx, drp_amd, torch, frames, seqs)
    q, held = _point_keys(ids, 64)
    flt = [drp_amd.make_filter(key_prefix=bytes(d)) for d in _key_digits(q)]
    stat = _timers(ctx, torch, dev, iters)
    rows = _row_tensors(torch, dev, 64)
    rb_t = torch.zeros(65, dtype=torch.int64, device=dev)
    foff = torch.zeros(65, dtype=torch.int64, device=dev)
    out = torch.zeros(64 * 86, dtype=torch.uint8, device=dev)
    tf = stat(lambda: ctx.fanout_device(store.arena, store.cols, store.max_keys, flt, rows, 64, None, rb_t))
    te = stat(lambda: ctx.encode_device(rows, store.arena, held, foff, out, out.numel()))
    assert int(rb_t.cpu()[64]) == held and int(foff[held].cpu()) == held * 86, "point read rows"
    return {"bench": "relay_lookup_baseline", "frames": n, "batch_rows": m, "keys": int(len(ids)), "seqs": seqs,
            "iters": iters, "merge_ms": merge_ms,
            "point_read_64": {"filters": 64, "rows_out": held, "fanout_ms": tf, "encode_ms": te,
                              "total_ms_median": tf["median"] + te["median"]}}


def _query_cols(torch, dev, nq, change):
    """Host-built query columns over a heap of ten-digit keys laid end to end: no wire, no decode."""
    i64 = lambda v: torch.full((nq,), v, dtype=torch.int64, device=dev)
    i32 = lambda v: torch.full((nq,), v, dtype=torch.int32, device=dev)
    return {"payload_off": torch.arange(nq, dtype=torch.int64, device=dev) * 10, "payload_len": i32(10),
            "type": torch.ones(nq, dtype=torch.uint8, device=dev), "flags": torch.zeros(nq, dtype=torch.uint8, device=dev),
            "key_off": i32(0), "key_len": i32(10), "subset_off": i32(10), "subset_len": i32(0), "value_off": i32(10),
            "value_len": i32(0), "change": i64(change), "from": i64(0), "to": i64(0)}


def lookup_leg(ctx, drp_amd, torch, frames, seqs, iters, parent=None):
    dev = torch.device("cuda", 0)
    store, ids, n, m, merge_ms = _lookup_store(ctx, drp_amd, torch, frames, seqs)
    keys = int(len(ids))
    stat = _timers(ctx, torch, dev, iters)
    ch = store.cols["change"][:keys].cpu().numpy()
    res = {"frames": n, "batch_rows": m, "keys": keys, "seqs": seqs, "iters": iters, "merge_ms": merge_ms,
           "sum_merge_ms": sum(x["median"] for x in merge_ms), "point": {}}
    z = lambda k, dt: torch.zeros(k, dtype=dt, device=dev)
    for nq in LOOKUP_SIZES:
        q, held = _point_keys(ids, nq)
        heap_t = torch.from_numpy(_key_digits(q).reshape(-1)).to(dev)
        qc = _query_cols(torch, dev, nq, HAVE_CHANGE)
        verdict, hit, counts, oq, n_out = z(nq, torch.uint8), z(nq, torch.int64), z(5, torch.int64), z(nq, torch.int64), z(1, torch.int64)
        rows = _row_tensors(torch, dev, nq)
        foff, out = z(held + 1, torch.int64), z(held * 86, torch.uint8)
        t_verdict = stat(lambda: ctx.store_lookup_device(store, heap_t, qc, nq, None, 0, verdict, hit, counts))
        t_get = stat(lambda: ctx.store_lookup_device(store, heap_t, qc, nq, None, drp_amd.LOOKUP_FOUND, verdict, hit, counts,
                                                     None, rows, oq, n_out, nq))
        t_enc = stat(lambda: ctx.encode_device(rows, store.arena, held, foff, out, out.numel()))
        cnt = [int(v) for v in counts.cpu()]
        assert cnt[0] == 0 and cnt[1] == nq - held and sum(cnt) == nq and int(n_out.cpu()[0]) == held, (cnt, held)
        found = hit.cpu().numpy()
        assert int((found >= 0).sum()) == held and int(foff[held].cpu()) == held * 86, "multi-get rows"
        # every hit row holds the queried key
        at = store.cols["payload_off"].cpu().numpy()[found[found >= 0]]
        got = store.arena.cpu().numpy()[at[:, None] + np.arange(10)[None, :]]
        assert np.array_equal(got, _key_digits(q)[found >= 0]), "hit rows"
        res["point"][f"n{nq}"] = {"queries": nq, "held": held, "verdict_ms": t_verdict, "multi_get_ms": t_get,
                                  "encode_ms": t_enc, "out_bytes": held * 86,
                                  "total_ms_median": t_get["median"] + t_enc["median"]}
        print("lookup", nq, res["point"][f"n{nq}"], file=sys.stderr, flush=True)
        heap_t = qc = rows = foff = out = None
        torch.cuda.empty_cache()
    # the have-list: every key of the store at change HAVE_CHANGE, then the select and encode of what the sender lacks
    nq = keys
    heap_t = torch.from_numpy(_key_digits(ids).reshape(-1)).to(dev)
    qc = _query_cols(torch, dev, nq, HAVE_CHANGE)
    counts, lack = z(5, torch.int64), z(keys, torch.uint8)
    t_have = stat(lambda: ctx.store_lookup_device(store, heap_t, qc, nq, None, 0, None, None, counts, lack))
    lacking = int((ch > HAVE_CHANGE).sum())
    cnt = [int(v) for v in counts.cpu()]
    assert cnt == [0, 0, int((ch < HAVE_CHANGE).sum()), int((ch == HAVE_CHANGE).sum()), lacking], cnt
    assert int(lack.count_nonzero().cpu()) == lacking, "lack_type"
    rows = _row_tensors(torch, dev, lacking)
    nsel = z(1, torch.int64)
    foff, out = z(lacking + 1, torch.int64), z(lacking * 86, torch.uint8)
    view = dict(store.cols, type=lack)
    t_sel = stat(lambda: ctx.select_device(store.arena, view, keys, None, rows, None, nsel))
    t_enc = stat(lambda: ctx.encode_device(rows, store.arena, lacking, foff, out, out.numel()))
    assert int(nsel.cpu()[0]) == lacking and int(foff[lacking].cpu()) == lacking * 86, "sync reply rows"
    res["have_list"] = {"queries": nq, "change": HAVE_CHANGE, "lacking_rows": lacking, "lookup_ms": t_have,
                        "select_ms": t_sel, "encode_ms": t_enc, "out_bytes": lacking * 86,
                        "total_ms_median": t_have["median"] + t_sel["median"] + t_enc["median"]}
    print("have-list", res["have_list"], file=sys.stderr, flush=True)
    if parent is not None:
        assert parent["frames"] == n and parent["keys"] == keys
        res["parent_merge_ms"] = parent["merge_ms"]
        res["sum_parent_merge_ms"] = sum(x["median"] for x in parent["merge_ms"])
        res["merge_inside_parent_spread"] = [p["min"] <= x["median"] <= p["max"]
                                             for x, p in zip(merge_ms, parent["merge_ms"])]
        res["parent_point_read_64"] = parent["point_read_64"]
        res["parent_point_read_over_multi_get_64"] = (parent["point_read_64"]["total_ms_median"] /
                                                      res["point"]["n64"]["total_ms_median"])
    return res


# ---- store lifecycle ---------------------------------------------------------------------------------

def lifecycle_leg(ctx, drp_amd, torch, frames, runs):
    """Moving a store: merge against load of its view into a fresh store, the rehash, and the compact
    and the init for scale (include/drp.h "store lifecycle")."""
    dev = torch.device("cuda", 0)
    store, keys, n = _final_store(ctx, drp_amd, torch, frames)
    stat = _timers(ctx, torch, dev, runs)
    used = int(store.query().arena_used)  # (the live bytes: _final_store's arena has room to spare)
    view = (store._view(), store.cols, store.max_keys)
    fresh = drp_amd.Store(ctx, keys, store.arena_bytes)
    clash_t = torch.zeros(1, dtype=torch.int64, device=dev)
    report_t = torch.zeros(2, dtype=torch.int64, device=dev)

    def merge():
        ctx.store_init(fresh)
        ctx.store_merge_device(fresh, *view)

    def load(clash):
        ctx.store_init(fresh)
        ctx.store_load_device(fresh, *view, None, clash)

    def filled():
        i = fresh.query()
        assert (i.rows, i.inserted, i.refused, i.arena_used) == (keys, keys, 0, used), i.as_dict()
        return {k: v.clone() for k, v in fresh.cols.items()}, fresh.arena.clone()

    res = {"keys": keys, "frames": n, "arena_used": used, "runs": runs}
    res["init_ms"] = stat(lambda: ctx.store_init(fresh))
    res["init_merge_ms"] = stat(merge)
    want_cols, want_arena = filled()
    for name, clash in [("init_load_ms", None), ("init_load_clash_ms", clash_t)]:
        res[name] = stat(lambda: load(clash))
        cols, arena = filled()
        assert torch.equal(arena, want_arena) and all(torch.equal(cols[k], want_cols[k]) for k in cols), name
    assert int(clash_t.cpu()[0]) == 0
    del want_cols, want_arena, cols, arena, fresh
    res["rehash_ms"] = stat(lambda: ctx.store_rehash_device(store))
    res["rehash_report_ms"] = stat(lambda: ctx.store_rehash_device(store, report_t))
    assert [int(v) for v in report_t.cpu()] == [0, 0] and int(torch.count_nonzero(store.table)) == keys
    assert store.query().refused == 0
    a2 = torch.zeros(store.arena_bytes, dtype=torch.uint8, device=dev)
    # (the store is compact already: every round copies each payload to the offset it has)
    res["compact_ms"] = stat(lambda: ctx.store_compact(store, a2))
    assert store.query().refused == 0
    res["load_over_merge"] = res["init_load_ms"]["median"] / res["init_merge_ms"]["median"]
    res["load_clash_over_merge"] = res["init_load_clash_ms"]["median"] / res["init_merge_ms"]["median"]
    res["load_not_slower_than_merge"] = bool(res["load_clash_over_merge"] <= 1.0 and res["load_over_merge"] <= 1.0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20_000_000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-mib", type=int, default=64)
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--probe", default=None, help="a built scripts/probe_bw.hip")
    ap.add_argument("--out", default=None)
    ap.add_argument("--fanout-out", default=None, help="run the fan-out legs too and write their JSON line here")
    ap.add_argument("--latest-out", default=None, help="run the latest-per-key legs too and write their JSON line here")
    ap.add_argument("--latest-only", action="store_true", help="with --latest-out: leave the other legs out")
    ap.add_argument("--fanout-latest-out", nargs="?", default=None,
                    const=os.path.join(ROOT, "profiles", "relay", "fanout_latest_bench.json"),
                    help="run the fan-out-of-latest legs too and write their JSON line here")
    ap.add_argument("--fanout-latest-only", action="store_true",
                    help="with --fanout-latest-out: leave the other legs out")
    ap.add_argument("--store-out", nargs="?", default=None,
                    const=os.path.join(ROOT, "profiles", "relay", "store_bench.json"),
                    help="run the store leg too and write its JSON line here")
    ap.add_argument("--store-only", action="store_true", help="with --store-out: leave the other legs out")
    ap.add_argument("--store-seqs", type=int, default=5, help="timed sequences of 8 merges")
    ap.add_argument("--store-baseline-out", default=None,
                    help="only drp_latest_device over the store leg's batches (any commit's library), written here")
    ap.add_argument("--store-baseline", default=None, help="such a file of the parent commit, read into the store leg's result")
    ap.add_argument("--digest-out", nargs="?", default=None,
                    const=os.path.join(ROOT, "profiles", "relay", "digest_bench.json"),
                    help="run the digest leg too and write its JSON line here")
    ap.add_argument("--digest-only", action="store_true", help="with --digest-out: leave the other legs out")
    ap.add_argument("--digest-baseline-out", default=None,
                    help="only the digest leg's yardsticks (compact, full snapshot; any commit's library), written here")
    ap.add_argument("--digest-baseline", default=None, help="such a file of the parent commit, read into the digest leg's result")
    ap.add_argument("--digest-refine-out", nargs="?", default=None,
                    const=os.path.join(ROOT, "profiles", "relay", "digest_refine_bench.json"),
                    help="run only the refined-digest leg and write its JSON line here")
    ap.add_argument("--digest-refine-baseline-out", default=None,
                    help="only the yardsticks and the single-level reconcile (any commit's library with the digest), written here")
    ap.add_argument("--digest-refine-baseline", default=None,
                    help="such a file of the parent commit, read into the refined-digest leg's result")
    ap.add_argument("--news-out", nargs="?", default=None, const=os.path.join(ROOT, "profiles", "relay", "news_bench.json"),
                    help="run the merge report leg alone (over the store leg's stream) and write its JSON line here")
    ap.add_argument("--news-baseline-out", default=None,
                    help="run the plain merges and the whole-batch relay alone (no call of this commit) and write them here")
    ap.add_argument("--news-baseline", default=None, help="such a file of the parent commit, read into the news leg's result")
    ap.add_argument("--order-out", nargs="?", default=None, const=os.path.join(ROOT, "profiles", "relay", "order_bench.json"),
                    help="run the ordered catch-up leg alone and write its JSON line here")
    ap.add_argument("--keyorder-out", nargs="?", default=None,
                    const=os.path.join(ROOT, "profiles", "relay", "keyorder_bench.json"),
                    help="run the key-ordered listing leg alone and write its JSON line here")
    ap.add_argument("--order-profile", action="store_true",
                    help="with --order-out: K = 64 and the plain drp_order_device calls alone (for a kernel trace)")
    ap.add_argument("--order-baseline-out", default=None,
                    help="only the order leg's yardstick (fan-out and encode over the final store) to this file")
    ap.add_argument("--order-baseline", default=None, help="such a file of the parent commit, read into the order leg's result")
    ap.add_argument("--lookup-out", nargs="?", default=None, const=os.path.join(ROOT, "profiles", "relay", "lookup_bench.json"),
                    help="run the lookup leg alone and write its JSON line here")
    ap.add_argument("--lookup-baseline-out", default=None,
                    help="only the point read by fan-out and the merge sequences (no call of this commit), written here")
    ap.add_argument("--lookup-baseline", default=None, help="such a file of the parent commit, read into the lookup leg's result")
    ap.add_argument("--lifecycle-out", nargs="?", default=None,
                    const=os.path.join(ROOT, "profiles", "relay", "lifecycle_bench.json"),
                    help="run the store lifecycle leg alone (load against merge, rehash, compact) and write its JSON line here")
    a = ap.parse_args()
    if a.digest_only and not a.digest_out:
        ap.error("--digest-only needs --digest-out")
    if a.store_only and not a.store_out:
        ap.error("--store-only needs --store-out")
    if a.latest_only and not a.latest_out:
        ap.error("--latest-only needs --latest-out")
    if a.fanout_latest_only and not a.fanout_latest_out:
        ap.error("--fanout-latest-only needs --fanout-latest-out")
    res = {"bench": "relay"}
    if a.probe:
        res["probe_bw"] = run_probe(a.probe)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_relay.py needs an MI355X")
    torch.cuda.init()
    import _streams as S
    import drp_amd
    if a.lifecycle_out:
        with drp_amd.Ctx(0) as ctx:
            lc = {"bench": "relay_lifecycle", "device": lifecycle_leg(ctx, drp_amd, torch, a.frames, a.runs)}
        with open(a.lifecycle_out, "w") as f:
            f.write(json.dumps(lc) + "\n")
        print(json.dumps(lc))
        return
    if a.lookup_baseline_out:
        with drp_amd.Ctx(0) as ctx:
            base = lookup_baseline(ctx, drp_amd, torch, a.frames, a.store_seqs, a.iters)
        with open(a.lookup_baseline_out, "w") as f:
            f.write(json.dumps(base) + "\n")
        print(json.dumps(base))
        return
    if a.lookup_out:
        parent = json.loads(open(a.lookup_baseline).read()) if a.lookup_baseline else None
        with drp_amd.Ctx(0) as ctx:
            lk = {"bench": "relay_lookup", "device": lookup_leg(ctx, drp_amd, torch, a.frames, a.store_seqs, a.iters, parent)}
        with open(a.lookup_out, "w") as f:
            f.write(json.dumps(lk) + "\n")
        print(json.dumps(lk))
        return
    if a.news_baseline_out:
        with drp_amd.Ctx(0) as ctx:
            base = news_baseline(ctx, drp_amd, torch, a.frames, a.store_seqs, a.iters)
        with open(a.news_baseline_out, "w") as f:
            f.write(json.dumps(base) + "\n")
        print(json.dumps(base))
        return
    if a.news_out:
        parent = json.loads(open(a.news_baseline).read()) if a.news_baseline else None
        with drp_amd.Ctx(0) as ctx:
            nw = {"bench": "relay_news", "device": news_leg(ctx, drp_amd, torch, a.frames, a.store_seqs, a.iters, parent)}
        with open(a.news_out, "w") as f:
            f.write(json.dumps(nw) + "\n")
        print(json.dumps(nw))
        return
    if a.keyorder_out:
        with drp_amd.Ctx(0) as ctx:
            ko = {"bench": "relay_keyorder", "device": keyorder_leg(ctx, drp_amd, torch, a.frames, a.iters)}
        with open(a.keyorder_out, "w") as f:
            f.write(json.dumps(ko) + "\n")
        print(json.dumps(ko))
        return
    if a.order_baseline_out:
        with drp_amd.Ctx(0) as ctx:
            base = order_baseline(ctx, drp_amd, torch, a.frames, a.iters)
        with open(a.order_baseline_out, "w") as f:
            f.write(json.dumps(base) + "\n")
        print(json.dumps(base))
        return
    if a.order_out:
        parent = json.loads(open(a.order_baseline).read()) if a.order_baseline else None
        assert parent is None or parent["frames"] == a.frames - a.frames % STORE_BATCHES
        with drp_amd.Ctx(0) as ctx:
            od = {"bench": "relay_order", "device": order_leg(ctx, drp_amd, torch, a.frames, a.iters, parent, a.order_profile)}
        with open(a.order_out, "w") as f:
            f.write(json.dumps(od) + "\n")
        print(json.dumps(od))
        return
    if a.digest_refine_baseline_out:
        with drp_amd.Ctx(0) as ctx:
            base = digest_refine_baseline(ctx, drp_amd, torch, a.frames, a.iters)
        with open(a.digest_refine_baseline_out, "w") as f:
            f.write(json.dumps(base) + "\n")
        print(json.dumps(base))
        return
    if a.digest_refine_out:
        parent = json.loads(open(a.digest_refine_baseline).read()) if a.digest_refine_baseline else None
        assert parent is None or parent["frames"] == a.frames
        with drp_amd.Ctx(0) as ctx:
            dr = {"bench": "relay_digest_refine",
                  "device": digest_refine_leg(ctx, drp_amd, torch, a.frames, a.iters, parent)}
        with open(a.digest_refine_out, "w") as f:
            f.write(json.dumps(dr) + "\n")
        print(json.dumps(dr))
        return
    if a.digest_baseline_out:
        with drp_amd.Ctx(0) as ctx:
            base = digest_baseline(ctx, drp_amd, torch, a.frames, a.iters)
        with open(a.digest_baseline_out, "w") as f:
            f.write(json.dumps(base) + "\n")
        print(json.dumps(base))
        return
    if a.digest_out:
        parent = json.loads(open(a.digest_baseline).read()) if a.digest_baseline else None
        assert parent is None or parent["frames"] == a.frames
        with drp_amd.Ctx(0) as ctx:
            dg = {"bench": "relay_digest", "device": digest_leg(ctx, drp_amd, torch, a.frames, a.iters, parent)}
        with open(a.digest_out, "w") as f:
            f.write(json.dumps(dg) + "\n")
        print(json.dumps(dg))
        if a.digest_only:
            return
    if a.store_baseline_out:
        with drp_amd.Ctx(0) as ctx:
            base = store_baseline(ctx, drp_amd, torch, a.frames, a.store_seqs)
        with open(a.store_baseline_out, "w") as f:
            f.write(json.dumps(base) + "\n")
        print(json.dumps(base))
        return
    if a.store_out:
        with drp_amd.Ctx(0) as ctx:
            st = {"bench": "relay_store", "device": store_leg(ctx, drp_amd, torch, a.frames, a.store_seqs, a.iters)}
        if a.store_baseline:
            parent = json.loads(open(a.store_baseline).read())
            d = st["device"]
            assert parent["frames"] == d["frames"] and parent["batch_rows"] == d["batch_rows"]
            d["parent_latest_alone_ms"] = parent["latest_alone_ms"]
            d["parent_latest_concat_ms"] = parent["latest_concat_ms"]
            d["merge_over_parent_latest_alone"] = [x["median"] / y["median"] for x, y in
                                                   zip(d["merge_ms"], parent["latest_alone_ms"])]
            d["parent_latest_concat_over_merge"] = [x["median"] / y["median"] for x, y in
                                                    zip(parent["latest_concat_ms"], d["merge_ms"])]
            d["sum_parent_latest_alone_ms"] = sum(x["median"] for x in parent["latest_alone_ms"])
            d["sum_parent_latest_concat_ms"] = sum(x["median"] for x in parent["latest_concat_ms"])
        with open(a.store_out, "w") as f:
            f.write(json.dumps(st) + "\n")
        print(json.dumps(st))
        if a.store_only:
            return
    if a.fanout_latest_out:
        with drp_amd.Ctx(0) as ctx:
            ctx.set_blob_skip(drp_amd.BLOB_SKIP_OFF)
            fl = {"bench": "relay_fanout_latest",
                  "device": fanout_latest_device_leg(ctx, drp_amd, torch, a.frames, a.iters),
                  "host": fanout_latest_host_leg(ctx, drp_amd, a.host_mib, a.runs)}
        with open(a.fanout_latest_out, "w") as f:
            f.write(json.dumps(fl) + "\n")
        print(json.dumps(fl))
        if a.fanout_latest_only:
            return
    if a.latest_out:
        with drp_amd.Ctx(0) as ctx:
            ctx.set_blob_skip(drp_amd.BLOB_SKIP_OFF)
            lat = {"bench": "relay_latest", "device": latest_device_leg(ctx, drp_amd, torch, a.frames, a.iters),
                   "host": latest_host_leg(ctx, drp_amd, a.host_mib, a.runs)}
            if a.probe:
                lat["probe_bw"] = res["probe_bw"]
        with open(a.latest_out, "w") as f:
            f.write(json.dumps(lat) + "\n")
        print(json.dumps(lat))
        if a.latest_only:
            return
    with drp_amd.Ctx(0) as ctx:
        ctx.set_blob_skip(drp_amd.BLOB_SKIP_OFF)
        decoded = device_setup(ctx, drp_amd, torch, S, a.frames)
        res["device"] = device_leg(ctx, drp_amd, torch, decoded, a.iters)
        if a.probe and "cols_rd" in res["probe_bw"]:
            res["device"]["over_cols_rd"] = res["device"]["model_TBps"] / res["probe_bw"]["cols_rd"]["TBps"]
        fan = None
        if a.fanout_out:
            fan = {"bench": "relay_fanout", "device": fanout_device_leg(ctx, drp_amd, torch, decoded, a.iters)}
        del decoded
        torch.cuda.empty_cache()
        res["host"] = host_leg(ctx, drp_amd, S, a.host_mib, a.runs)
        if fan is not None:
            fan["host"] = fanout_host_leg(ctx, drp_amd, S, a.host_mib, a.runs)
            with open(a.fanout_out, "w") as f:
                f.write(json.dumps(fan) + "\n")
            print(json.dumps(fan))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
