"""GPU parity of the Change encoder (csrc/drp_encode.hip, drp_encode_device) with the oracle's
encode.js + protocol-buffers@2 restatement (_oracle.encode_changes), byte for byte, at the states
the writer's address arithmetic can go wrong in: row counts around the scan's block edges and past
one round of the block-sum scan, headers and length prefixes of one to five varint bytes, frames
over many 64 KiB output blocks, the switch between the block writer and the per-frame writer at
ENC_FMAX = 128 frames a block, field lengths around the 16-byte chunk edges under both writers,
wave_copy's vector path at every pair of source and destination alignments, drp_encode_device's own
contract (capacity, ranges, absent fields, flag bits) and the round trip through the decode and the
relay. Every wire is written at an output address of every alignment mod 16 (`shift`) into a buffer
of guard bytes. tests/_encode.py builds the cases; tests/test_encode_cases.py proves on the CPU that
each one reaches the blocks, widths and writers it is named for.

Not pinned here: frames of 2^31 bytes or more (enc_write_os hands them to the per-frame writer, one
wave copying gigabytes) and the branch taken when a block lists more than ENC_MIXCAP mixed chunks
(the bound is not reached by any layout of at most 128 frames)."""
import ctypes as C

import numpy as np
import pytest

import _encode as E
import _oracle as O
import _streams as S

pytestmark = pytest.mark.gpu

SHIFTS = range(16)


@pytest.fixture(scope="module")
def ctx():
    from _gpu import drp_amd
    c = drp_amd.Ctx(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def dev():
    import torch
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def long0(dev):
    """long_fields(0) on the device: shared by the encode and the round-trip tests."""
    return E.DevCase(E.long_fields(0), dev)


# ---- 1. row counts ------------------------------------------------------------------------------

@pytest.mark.parametrize("n", E.SMALL_COUNTS)
def test_row_counts(ctx, dev, n):
    """Mixed short rows around the wave, the 1024-row scan block and its multiples: the wire, the
    guard bytes and every frame_off[0..n]. n = 0: frame_off[0] = 0 and nothing else is touched."""
    d = E.DevCase(E.mixed_short(n, seed=10 + n), dev)
    for shift in (0, 5, 15):
        d.check(ctx, shift, label=f"n={n}")
    d.check(ctx, 3, cap=d.W, label=f"n={n} cap=W")


def test_rows_past_one_scan_round(ctx, dev):
    """2^20 + 2 rows: 1025 per-block sums, so enc_blocksum_kernel scans a second round of 1024 and
    carries the first round's total into it; the last row (a key and a value) lies in that round."""
    d = E.DevCase(E.past_one_scan_round(), dev)
    d.check(ctx, 0, label="2^20+2")
    d.check(ctx, 11, cap=d.W, label="2^20+2 cap=W")


# ---- 2. varint widths ---------------------------------------------------------------------------

def test_header_and_prefix_varint_widths(ctx, dev):
    """Frame headers of 1, 2, 3 and 4 bytes on both sides of each step, and a 1-, 2-, 3- and 4-byte
    length prefix in every prefix slot (subset: LIT0, key: LIT2, value: LIT4)."""
    d = E.DevCase(E.varint_widths(), dev)
    for shift in SHIFTS:
        d.check(ctx, shift, label="varint widths")


def test_five_byte_varints(ctx, dev):
    """A value of 2^28 bytes, the smallest whose prefix and frame header take five bytes, between two
    short rows: the heap is made on the device, the frame's leading bytes are compared with varint
    arithmetic and its body with the heap on the device."""
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(28)
    VL = 1 << 28
    heap = torch.randint(0, 256, (VL + 64,), generator=g, device=dev, dtype=torch.uint8)
    # row 0: key heap[0:3], value heap[3:8]; row 1: key heap[8:15], value heap[21:21 + 2^28]; row 2: key heap[15:21]
    cols = {"key_off": [0, 8, 15], "key_len": [3, 7, 6], "subset_off": [0, 0, 0], "subset_len": [0, 0, 0],
            "value_off": [3, 21, 0], "value_len": [5, VL, 0], "change": [1, 1 << 60, 3], "from": [0, 200, 0],
            "to": [9, 2, 1], "flags": [2, 2, 0]}
    dt = lambda k: torch.uint8 if k == "flags" else torch.int32 if k.endswith("_len") else torch.int64
    ct = {k: torch.tensor(v, dtype=dt(k), device=dev) for k, v in cols.items()}
    head = heap[:32].cpu().numpy().tobytes()
    f0 = S.frame(S.change_payload(head[0:3], 1, 0, 9, value=head[3:8]))
    f2 = S.frame(S.change_payload(head[15:21], 3, 0, 1))
    pre = S.change_payload(head[8:15], 1 << 60, 200, 2) + b"\x32" + S.varint(VL)
    lead = S.varint(len(pre) + VL + 1) + b"\x01" + pre
    assert len(S.varint(VL)) == 5 and len(S.varint(len(pre) + VL + 1)) == 5
    W = len(f0) + len(lead) + VL + len(f2)
    wire, foff, (gh, gt) = E.run_encode(ctx, ct, heap, 3, W, 3, cap=W)
    assert foff.tolist() == [0, len(f0), len(f0) + len(lead) + VL, W]
    a = len(f0) + len(lead)
    assert wire[:a].cpu().numpy().tobytes() == f0 + lead
    assert wire[a + VL:].cpu().numpy().tobytes() == f2
    assert torch.equal(wire[a:a + VL], heap[21:21 + VL])
    assert bool((gh == E.GUARD).all()) and bool((gt == E.GUARD).all())


# ---- 3. long fields across blocks ---------------------------------------------------------------

@pytest.mark.parametrize("mis", range(16))
def test_long_fields_across_blocks(ctx, dev, long0, mis):
    """Values of 70 000, 200 000 and 2^21 bytes, a key of 70 000 and a subset of 70 001 at heap offset
    `mis` mod 16, written at every output alignment: frames over 2 to 33 blocks, blocks wholly inside
    one copy, frame-relative offsets past 16 bits."""
    d = long0 if mis == 0 else E.DevCase(E.long_fields(mis), dev)
    for shift in SHIFTS:
        d.check(ctx, shift, label=f"long fields, source {mis}")


@pytest.mark.parametrize("where", ["behind", "before"])
@pytest.mark.parametrize("mis", [0, 7])
def test_long_fields_next_to_dense_blocks(ctx, dev, where, mis):
    """The long rows directly behind / before 300 ten-byte frames: the per-frame writer rewrites the
    long frame (all of it) for the dense block at one end, the block writer writes its other blocks."""
    kw = {"tiny_behind": 300} if where == "behind" else {"tiny_before": 300}
    d = E.DevCase(E.long_fields(mis, **kw), dev)
    for shift in SHIFTS:
        d.check(ctx, shift, label=f"long fields {where} tiny frames, source {mis}")


# ---- 4. the switch between the writers ----------------------------------------------------------

def test_block_switch_128_129(ctx, dev):
    """Runs of frames of one size, 504 to 528 bytes: blocks of 127, 128 (the LDS layout's last row),
    129 and more frames next to each other, so both writers meet at block edges in every run."""
    d = E.DevCase(E.block_switch(), dev)
    for shift in SHIFTS:
        d.check(ctx, shift, label="128/129 switch")


# ---- 5. chunk-edge field lengths ----------------------------------------------------------------

@pytest.mark.parametrize("writer", ["dense", "block"])
def test_chunk_edge_field_lengths(ctx, dev, writer):
    """Key, subset and value of 0, 1, 15, 16, 17, 31, 32 and 33 bytes in every combination, present and
    absent, numbers of 1 and 10 bytes. dense: alone (the per-frame writer); block: a 1030-byte-value
    row after each, so the block writer lays them out and most of their chunks are mixed ones."""
    d = E.DevCase(E.chunk_edges(writer == "block"), dev)
    for shift in SHIFTS:
        d.check(ctx, shift, label=f"chunk edges, {writer} writer")


# ---- 6. wave_copy's vector path -----------------------------------------------------------------

@pytest.mark.parametrize("mis", range(16))
def test_wave_copy_alignments(ctx, dev, mis):
    """Fields of 127 to 400 bytes inside dense blocks, as key, subset and value, at source alignment
    `mis` and (through the 16 output alignments) every destination alignment: the byte head, the
    funnel shift and the byte tail of wave_copy."""
    d = E.DevCase(E.wave_copy_rows(mis), dev)
    for shift in SHIFTS:
        d.check(ctx, shift, label=f"wave_copy, source {mis}")


# ---- 7. drp_encode_device's contract ------------------------------------------------------------

def _contract_case():
    """Dense blocks, a frame over four blocks (two of them the block writer's), short mixed rows, and a
    last row whose 400-byte value ends the heap and (in a dense block: wave_copy's tail) the wire."""
    rng = np.random.default_rng(70)
    m = 40
    kl = np.concatenate([np.zeros(300, int), [9], rng.integers(0, 41, m), np.zeros(300, int), [0, 4]])
    sl = np.concatenate([np.zeros(300, int), [2], rng.integers(0, 41, m), np.zeros(300, int), [0, 0]])
    vl = np.concatenate([np.zeros(300, int), [200_000], rng.integers(0, 41, m), np.zeros(300, int), [0, 400]])
    fl = np.concatenate([np.zeros(300, int), [3], rng.integers(0, 4, m), np.zeros(300, int), [0, 2]])
    return E.build(kl, sl, vl, fl, 1, seed=70)


def _untouched(ctx, d, shift, cap, heap_bytes=None, ct=None):
    """An encode that must write nothing: returns frame_off."""
    import torch
    wire, foff, (gh, gt) = E.run_encode(ctx, ct or d.ct, d.ht, d.n, d.W, shift, cap=cap, heap_bytes=heap_bytes)
    for t in (wire, gh, gt):
        assert bool((t == E.GUARD).all()), (shift, cap)
    return foff


def test_capacity(ctx, dev, long0):
    """cap == W: everything is written, nothing after it. cap == W - 1 and cap == 0: nothing is
    written, frame_off[0..n] is still the scan of the sizes and frame_off[n] == W."""
    import torch
    for d in (E.DevCase(_contract_case(), dev), long0):
        for shift in SHIFTS:
            d.check(ctx, shift, cap=d.W, label="cap == W")
        for cap in (d.W - 1, 0):
            for shift in (0, 9):
                foff = _untouched(ctx, d, shift, cap)
                assert torch.equal(foff, d.foff_t), cap
        d.check(ctx, 0, label="after a refused capacity")


def test_sizes_only(ctx, dev):
    """out == NULL: frame_off alone."""
    import torch
    from _gpu import drp_amd
    d = E.DevCase(_contract_case(), dev)
    foff = torch.full((d.n + 1,), -7, dtype=torch.int64, device=dev)
    tp = lambda t: C.c_void_p(t.data_ptr())
    src = drp_amd.ChangeSrc(*[tp(d.ct[k]) for k in E.SRC_COLS])
    torch.cuda.synchronize(dev)
    for heap, hb, cap in [(tp(d.ht), d.ht.numel(), 0), (None, 2**64 - 1, 2**64 - 1)]:
        foff.fill_(-7)
        torch.cuda.synchronize(dev)
        rc = ctx.L.drp_encode_device(ctx.h, C.byref(src), heap, hb, d.n, tp(foff), None, cap)
        assert rc == 0
        ctx.order_torch_after(foff)
        torch.cuda.synchronize(dev)
        assert torch.equal(foff, d.foff_t)


def test_heap_ranges(ctx, dev):
    """A range ending exactly at heap_bytes and a zero-length key at off == heap_bytes are accepted;
    a present field one byte past the heap poisons the total (frame_off[n] == 2^64 - 1), nothing is
    written, and the next call on the ctx works."""
    import torch
    c = _contract_case()
    hb = len(c.heap) - 16  # the last row's value ends here
    assert int(c.cols["value_off"][-1]) + int(c.cols["value_len"][-1]) == hb
    assert c.cols["key_len"][-2] == 0
    c.cols["key_off"][-2] = hb
    d = E.DevCase(c, dev)
    wire, foff, (gh, gt) = E.run_encode(ctx, d.ct, d.ht, d.n, d.W, 6, cap=d.W, heap_bytes=hb)
    assert torch.equal(foff, d.foff_t) and torch.equal(wire, d.exp_t)
    assert bool((gh == E.GUARD).all()) and bool((gt == E.GUARD).all())
    for name, row in [("value", d.n - 1), ("key", d.n - 1), ("subset", 300)]:
        ct = dict(d.ct)
        ct[name + "_off"] = d.ct[name + "_off"].clone()
        ct[name + "_off"][row] = hb + 1 - int(c.cols[name + "_len"][row])
        foff = _untouched(ctx, d, 6, d.W + 32, heap_bytes=hb, ct=ct)
        assert int(foff[d.n]) == -1, name  # 2^64 - 1
        d.check(ctx, 6, label="after a refused range")


def test_absent_fields_are_not_read(ctx, dev):
    """Offsets and lengths of an absent subset or value may hold anything."""
    c = E.mixed_short(3000, seed=71)
    d = E.DevCase(c, dev)
    no_s, no_v = (c.cols["flags"] & 1) == 0, (c.cols["flags"] & 2) == 0
    assert no_s.sum() > 500 and no_v.sum() > 500
    g = {k: v.copy() for k, v in c.cols.items()}
    rng = np.random.default_rng(72)
    for name, absent in (("subset", no_s), ("value", no_v)):
        g[name + "_off"][absent] = rng.integers(1 << 62, 1 << 63, int(absent.sum()), dtype=np.uint64) * np.uint64(2)
        g[name + "_len"][absent] = rng.integers(1 << 20, 1 << 32, int(absent.sum()), dtype=np.uint64).astype(np.uint32)
        g[name + "_len"][np.flatnonzero(absent)[:3]] = 0xFFFFFFFF
        g[name + "_off"][np.flatnonzero(absent)[:3]] = np.uint64(2**64 - 1)
    d.ct, _ = E.to_device(E.Case(c.heap, g), dev)
    for shift in (0, 1, 8, 15):
        d.check(ctx, shift, label="garbage in absent fields")


def test_other_flag_bits_ignored(ctx, dev):
    """Flag bits beyond DRP_F_SUBSET | DRP_F_VALUE (a decode's key flags, DRP_F_BAD's neighbours) on
    some rows: the wire of the same rows with the flags masked."""
    for c in (E.mixed_short(3000, seed=73), E.chunk_edges(True)):
        rng = np.random.default_rng(74)
        c.cols["flags"] |= (rng.integers(0, 64, c.n) << 2).astype(np.uint8) * (rng.random(c.n) < 0.5)
        assert (c.cols["flags"] > 3).sum() > c.n // 4
        d = E.DevCase(c, dev)  # (Case.exp: the oracle's wire of the masked flags)
        for shift in (0, 7):
            d.check(ctx, shift, label="other flag bits")


def test_encode_batch_pointer_kinds(ctx, dev):
    """drp_encode_batch through the C ABI: host columns and a host heap into a device `out`; device
    columns and a host heap into a host `out`. cap == W both times, guard bytes around."""
    import torch
    from _gpu import drp_amd
    c = _contract_case()
    d = E.DevCase(c, dev)
    W, exp = d.W, np.frombuffer(c.exp, np.uint8)
    hp = lambda a: C.c_void_p(a.ctypes.data)
    tp = lambda t: C.c_void_p(t.data_ptr())
    written = C.c_uint64()
    # host columns, host heap, device out
    buf = torch.full((W + 64,), E.GUARD, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    src = drp_amd.ChangeSrc(*[hp(c.cols[k]) for k in E.SRC_COLS])
    rc = ctx.L.drp_encode_batch(ctx.h, C.byref(src), hp(c.heap), len(c.heap), c.n, tp(buf[21:]), W, C.byref(written))
    assert (rc, written.value) == (0, W)
    got = buf.cpu().numpy()
    np.testing.assert_array_equal(got[21:21 + W], exp)
    assert (got[:21] == E.GUARD).all() and (got[21 + W:] == E.GUARD).all()
    # device columns, host heap, host out
    out = np.full(W + 64, E.GUARD, np.uint8)
    src = drp_amd.ChangeSrc(*[tp(d.ct[k]) for k in E.SRC_COLS])
    rc = ctx.L.drp_encode_batch(ctx.h, C.byref(src), hp(c.heap), len(c.heap), c.n, hp(out[21:]), W, C.byref(written))
    assert (rc, written.value) == (0, W)
    np.testing.assert_array_equal(out[21:21 + W], exp)
    assert (out[:21] == E.GUARD).all() and (out[21 + W:] == E.GUARD).all()
    # one byte short: DRP_E_CAPACITY, the size needed, nothing written
    out[:] = E.GUARD
    rc = ctx.L.drp_encode_batch(ctx.h, C.byref(src), hp(c.heap), len(c.heap), c.n, hp(out[21:]), W - 1, C.byref(written))
    assert (rc, written.value) == (drp_amd.DRP_E_CAPACITY, W) and (out == E.GUARD).all()


# ---- 8. round trip and relay --------------------------------------------------------------------

def _decode_device(ctx, dev, wire, n):
    import torch
    import bench
    from _gpu import drp_amd
    outs = bench.alloc_outputs(n + 64, dev)
    res = torch.zeros(C.sizeof(drp_amd.StreamResult), dtype=torch.uint8, device=dev)
    so = torch.tensor([0, wire.numel()], dtype=torch.int64, device=dev)
    ctx.decode_device(wire, so, None, outs, n + 64, res)
    torch.cuda.synchronize(dev)
    r = drp_amd.StreamResult.from_buffer_copy(res.cpu().numpy().tobytes())
    g = {k: v[:r.frames].cpu().numpy() for k, v in outs.items()}
    g.update(nframes=r.frames, err_code=r.err_code, err_detail=r.err_detail, consumed=r.consumed,
             tail=r.tail_kind, blob_remaining=r.blob_remaining, err_frame=r.err_frame)
    return g, outs


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("layout", ["plain", "behind"])
def test_round_trip_long_frames(ctx, dev, long0, layout, exact):
    """The long-field wire through drp_decode_device (the default path and the exact kernel): the
    oracle's rows, the encoder's input, and every field's bytes at payload_off + *_off equal to the
    heap's (long fields in full, on the device)."""
    import torch
    from _gpu import assert_same
    d = long0 if layout == "plain" else E.DevCase(E.long_fields(5, tiny_behind=300), dev)
    c = d.case
    wire = d.check(ctx, 0, label="round trip").clone()
    ctx.set_exact(exact)
    try:
        g, outs = _decode_device(ctx, dev, wire, d.n)
    finally:
        ctx.set_exact(False)
    assert_same(g, O.decode_batch(c.exp, cap=d.n + 2), f"{layout} exact={exact}")
    assert g["nframes"] == d.n and g["consumed"] == d.W and (g["type"] == 1).all()
    fl = c.cols["flags"]
    np.testing.assert_array_equal(g["flags"] & 3, fl)
    for k in ("change", "from", "to"):
        np.testing.assert_array_equal(g[k].view(np.uint64), c.cols[k])
    np.testing.assert_array_equal(g["key_len"], c.cols["key_len"])
    np.testing.assert_array_equal(g["subset_len"], np.where(fl & 1, c.cols["subset_len"], 0))
    np.testing.assert_array_equal(g["value_len"], np.where(fl & 2, c.cols["value_len"], 0))
    np.testing.assert_array_equal(g["payload_off"] + g["payload_len"], c.frame_off[1:].astype(np.int64))
    for row in np.flatnonzero(c.cols["key_len"] + c.cols["subset_len"] + c.cols["value_len"]):
        for name, bit in (("key", 0), ("subset", 1), ("value", 2)):
            ln = int(g[name + "_len"][row])
            if bit and not fl[row] & bit:
                continue
            at, src = int(g["payload_off"][row]) + int(g[name + "_off"][row]), int(c.cols[name + "_off"][row])
            assert torch.equal(wire[at:at + ln], d.ht[src:src + ln]), (row, name)


@pytest.mark.parametrize("layout", ["plain", "behind", "before"])
def test_relay_reproduces_long_frames(ctx, layout):
    """decode_staged + relay_staged with the empty filter over the long-field wire: the frames are
    canonical, so select's re-encode with the staged wire as the heap returns them byte for byte."""
    from _gpu import drp_amd
    kw = {"plain": {}, "behind": {"tiny_behind": 300}, "before": {"tiny_before": 300}}[layout]
    c = E.long_fields(11, **kw)
    st = ctx.decode_staged(c.exp)
    assert st["nframes"] == c.n and st["err_code"] == 0 and st["tail"] == 0
    out, nsel = ctx.relay_staged(drp_amd.make_filter())
    assert nsel == c.n and len(out) == len(c.exp)
    if out != c.exp:
        a, b = np.frombuffer(out, np.uint8), np.frombuffer(c.exp, np.uint8)
        i = int(np.flatnonzero(a != b)[0])
        raise AssertionError(f"relay of {layout}: byte {i} is {a[i]:#04x}, expected {b[i]:#04x}")
