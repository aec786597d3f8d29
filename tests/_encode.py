"""Case builders for the Change encoder's tests (csrc/drp_encode.hip): tests/test_encode_cases.py
proves on the CPU that every case reaches the state it is named for, tests/test_gpu_encode.py runs
the cases through drp_encode_device against the oracle (_oracle.encode_changes), byte for byte."""
import numpy as np

import _oracle as O

ENC_BS = 65536   # csrc/drp_encode.hip DRP_ENC_BS: bytes of one output block
ENC_FMAX = 128   # csrc/drp_encode.hip ENC_FMAX: frames a block may touch and still be laid out in LDS

F_SUBSET, F_VALUE = 1, 2
SRC_COLS = ["key_off", "key_len", "subset_off", "subset_len", "value_off", "value_len", "change", "from", "to",
            "flags"]
EDGE_LENS = [0, 1, 15, 16, 17, 31, 32, 33]              # around the 16-byte chunk edges
WAVE_LENS = [127, 128, 129, 143, 144, 145, 255, 256, 257, 400]  # around wave_copy's 128-byte threshold
LONG_ROWS = [("value", 70_000), ("value", 200_000), ("value", 1 << 21), ("key", 70_000), ("subset", 70_001)]
SWITCH_SIZES = range(504, 529)                           # frame bytes around ENC_BS / ENC_FMAX = 512
SMALL_COUNTS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049]
FIELD = {"key": 0, "subset": 1, "value": 2}


def vlen(v):
    """Bytes of the varint of v (a Python int)."""
    n = 1
    while v >= 0x80:
        v >>= 7
        n += 1
    return n


class Case:
    """A heap and the ten drp_change_src columns (numpy); the oracle's wire and frame offsets of it."""

    def __init__(self, heap, cols, rows=None):
        self.heap, self.cols, self.n = heap, cols, len(cols["key_len"])
        self.rows = rows if rows is not None else {}  # the rows a case is about, by name
        self._exp = self._foff = None

    @property
    def exp(self):
        if self._exp is None:
            c = dict(self.cols, flags=self.cols["flags"] & np.uint8(F_SUBSET | F_VALUE))
            self._exp = O.encode_changes(self.heap, c)
        return self._exp

    @property
    def frame_off(self):
        """frame_off[0..n] of the oracle's wire: the exclusive cumulative sum of its frame sizes, read
        from the oracle's own decode of it (a frame ends where its payload does)."""
        if self._foff is None:
            if self.n == 0:
                self._foff = np.zeros(1, np.uint64)
            else:
                d = O.decode_batch(self.exp, cap=self.n + 2)
                assert d["nframes"] == self.n and d["err_code"] == 0 and d["tail"] == 0
                ends = d["payload_off"].astype(np.uint64) + d["payload_len"].astype(np.uint64)
                self._foff = np.concatenate([np.zeros(1, np.uint64), ends])
        return self._foff


def build(key_len, subset_len, value_len, flags, numbers, pad=None, seed=0):
    """Rows with the given field lengths, flags and numbers ((3, n) or one int for all): each row's
    key, subset and value bytes lie end to end (in that order, absent fields too) in a seeded random
    heap with 16 spare bytes; pad[i] unused bytes lie before row i."""
    kl, sl, vl = (np.asarray(a, dtype=np.uint32) for a in (key_len, subset_len, value_len))
    n = len(kl)
    pad = np.zeros(n, np.uint64) if pad is None else np.asarray(pad, dtype=np.uint64)
    row = pad + kl + sl + vl
    base = (np.cumsum(row) - row + pad).astype(np.uint64)
    heap = np.random.default_rng(seed).integers(0, 256, int(row.sum()) + 16, dtype=np.uint8)
    nums = np.broadcast_to(np.asarray(numbers, dtype=np.uint64), (3, n))
    cols = {"key_off": base, "key_len": kl, "subset_off": base + kl, "subset_len": sl,
            "value_off": base + kl + sl, "value_len": vl, "change": nums[0].copy(), "from": nums[1].copy(),
            "to": nums[2].copy(), "flags": np.asarray(flags, dtype=np.uint8).copy()}
    return Case(heap, cols)


def pads_for(key_len, subset_len, value_len, placed, mis):
    """The per-row pad that puts the heap offset of field `placed[i]` ("key" / "subset" / "value") of
    every row i in `placed` at `mis` mod 16 (rows not in `placed`: no pad)."""
    n = len(key_len)
    pad = np.zeros(n, np.uint64)
    row = np.asarray(key_len, np.uint64) + np.asarray(subset_len, np.uint64) + np.asarray(value_len, np.uint64)
    before = np.cumsum(row) - row
    added = 0
    for i in sorted(placed):
        d = [0, int(key_len[i]), int(key_len[i]) + int(subset_len[i])][FIELD[placed[i]]]
        pad[i] = (mis - (int(before[i]) + added + d)) % 16
        added += int(pad[i])
    return pad


def frames_touching(frame_off, shift):
    """The number of frames enc_write_os lays out for each output block of a wire written at an
    address `shift` mod 16 (its f1 - f0): block b covers the wire bytes [b * ENC_BS - shift,
    (b + 1) * ENC_BS - shift); f0 is the frame holding the block's first byte and the frame holding
    the next block's first byte counts too, also when it starts exactly at the block's end."""
    fo = np.asarray(frame_off, dtype=np.int64)
    n, W = len(fo) - 1, int(fo[-1])
    nb = (W + shift + ENC_BS - 1) // ENC_BS
    first = np.arange(nb + 1, dtype=np.int64) * ENC_BS - shift
    owner = np.searchsorted(fo[:n], np.maximum(first, 0), side="right") - 1
    f1 = np.where(first[1:] < W, np.minimum(owner[1:] + 1, n), n)
    return f1 - owner[:nb]


def block_of(frame_off, shift, row):
    """The output blocks frame `row` has bytes in."""
    lo, hi = int(frame_off[row]) + shift, int(frame_off[row + 1]) + shift
    return range(lo // ENC_BS, (hi - 1) // ENC_BS + 1)


# ---- the cases --------------------------------------------------------------------------------

def tiny_rows(n):
    """n rows of ten-byte frames: no key bytes, no subset, no value, numbers below 128."""
    z = np.zeros(n, np.uint32)
    return z, z, z, np.zeros(n, np.uint8)


def mixed_short(n, seed=1):
    """n short rows of every flag combination, fields of 0..40 bytes, a number in seven at 2^64 - 1."""
    rng = np.random.default_rng(seed)
    nums = rng.integers(0, 1 << 40, (3, n), dtype=np.uint64)
    nums[:, ::7] = np.uint64(2**64 - 1)
    return build(rng.integers(0, 41, n), rng.integers(0, 41, n), rng.integers(0, 41, n),
                 rng.integers(0, 4, n), nums, seed=seed)


def past_one_scan_round():
    """2^20 + 1 empty rows without a value, then one row with a key and a value: 1025 per-block sums,
    so enc_blocksum_kernel's second round of 1024 runs and its carry places the last frame."""
    n = (1 << 20) + 2
    kl, sl, vl, fl = (a.copy() for a in tiny_rows(n))
    kl[-1], vl[-1], fl[-1] = 5, 37, F_VALUE
    nums = np.zeros((3, n), np.uint64)
    nums[:, -1] = [1 << 40, 300, 7]
    return build(kl, sl, vl, fl, nums, seed=2)


def key_len_for_frame_payload(p1):
    """The key length of a key-only row with one-byte numbers whose payload + 1 is p1."""
    for v in range(1, 6):
        kl = p1 - 1 - 7 - v  # payload = 0x12 + varint(kl) + kl + three (tag, number) pairs
        if kl >= 0 and vlen(kl) == v:
            return kl
    raise ValueError(p1)


VARINT_P1 = [127, 128, 16383, 16384, (1 << 21) - 1, 1 << 21]
VARINT_LENS = [127, 128, 16383, 16384, 1 << 21]


def varint_widths():
    """Key-only rows whose payload + 1 sits on either side of each header width up to four bytes, then
    for key, subset and value a row of each length around the prefix widths, short rows between.
    rows["header"]: row -> payload + 1; rows["prefix"]: row -> (field, length)."""
    kl, sl, vl, fl, hdr, pre = [], [], [], [], {}, {}

    def add(k, s, v, f):
        kl.append(k), sl.append(s), vl.append(v), fl.append(f)
        kl.append(3), sl.append(2), vl.append(4), fl.append(len(kl) // 2 % 4)  # a short row after it
        return len(kl) - 2

    for p1 in VARINT_P1:
        hdr[add(key_len_for_frame_payload(p1), 0, 0, 0)] = p1
    for field in ("key", "subset", "value"):
        for ln in VARINT_LENS:
            k, s, v = (ln if field == f else 9 for f in ("key", "subset", "value"))
            pre[add(k, s, v, F_SUBSET | F_VALUE)] = (field, ln)
    c = build(kl, sl, vl, fl, 5, seed=3)
    c.rows = {"header": hdr, "prefix": pre}
    return c


def long_fields(mis=0, tiny_behind=0, tiny_before=0):
    """The LONG_ROWS with short rows between them, every long field at heap offset `mis` mod 16.
    tiny_behind / tiny_before: that many ten-byte frames directly before / after every long row (a
    dense block then rewrites part of a frame that sparse blocks also write). rows["long"]: row ->
    (field, length)."""
    kl, sl, vl, fl, placed, long_ = [], [], [], [], {}, {}

    def add(k, s, v, f, times=1):
        for _ in range(times):
            kl.append(k), sl.append(s), vl.append(v), fl.append(f)

    add(20, 3, 50, 3)
    for field, ln in LONG_ROWS:
        add(0, 0, 0, 0, tiny_behind)
        k, s, v = (ln if field == f else 11 for f in ("key", "subset", "value"))
        add(k, s, v, F_SUBSET | F_VALUE)
        placed[len(kl) - 1] = field
        long_[len(kl) - 1] = (field, ln)
        add(0, 0, 0, 0, tiny_before)
        add(20, 3, 50, len(kl) % 4)
    n = len(kl)
    nums = np.random.default_rng(4).integers(0, 1 << 50, (3, n), dtype=np.uint64)
    nums[:, np.array(kl) == 0] = 1
    c = build(kl, sl, vl, fl, nums, pad=pads_for(kl, sl, vl, placed, mis), seed=4)
    c.rows = {"long": long_}
    return c


def block_switch(per_size=700):
    """per_size rows of one frame size for each size in SWITCH_SIZES, one run after another: around
    512-byte frames a block touches 127 to 131 of them, so both writers run on neighbouring blocks."""
    sizes = np.repeat(np.array(SWITCH_SIZES), per_size)
    n = len(sizes)
    # header 2 + type 1 + key 0x12 01 k(8) + numbers 6 + value 0x32 vv v: 22 bytes around the value
    vl = sizes - 22
    rng = np.random.default_rng(5)
    c = build(np.full(n, 8), np.zeros(n, int), vl, np.full(n, F_VALUE), rng.integers(0, 128, (3, n)), seed=5)
    c.rows = {"size": sizes}
    return c


def chunk_edges(filler):
    """Every (key, subset, value) length over EDGE_LENS^3, with each flag combination and numbers of 1
    and 10 varint bytes: 4096 frames of 10 to ~170 bytes (dense blocks). filler: a row with a
    1030-byte value after every row, so that no block touches more than ENC_FMAX frames and the
    block writer assembles them as mixed chunks. rows["edge"]: the rows of the product."""
    L = np.array(EDGE_LENS)
    k, s, v, f, w = (a.reshape(-1) for a in np.meshgrid(L, L, L, np.arange(4), np.arange(2), indexing="ij"))
    # spread the shortest frames (no optional field) between the others
    order = np.random.default_rng(6).permutation(len(k))
    k, s, v, f, w = (a[order] for a in (k, s, v, f, w))
    num = np.where(w == 1, np.uint64(2**64 - 1), np.uint64(3))
    edge = np.arange(len(k))
    if filler:
        m = 2 * len(k)
        kk, ss, vv, ff = np.full(m, 8), np.zeros(m, int), np.full(m, 1030), np.full(m, F_VALUE)
        nn = np.full(m, 77, np.uint64)
        edge = edge * 2
        kk[edge], ss[edge], vv[edge], ff[edge], nn[edge] = k, s, v, f, num
        k, s, v, f, num = kk, ss, vv, ff, nn
    c = build(k, s, v, f, num, seed=6)
    c.rows = {"edge": edge}
    return c


def wave_copy_rows(mis=0, run=200):
    """Runs of `run` ten-byte frames (dense blocks, so the per-frame writer's wave_copy) around one row
    per (field, length in WAVE_LENS), that field at heap offset `mis` mod 16. rows["wave"]: row ->
    (field, length)."""
    kl, sl, vl, fl, placed, rows = [], [], [], [], {}, {}
    for field in ("key", "subset", "value"):
        for ln in WAVE_LENS:
            for _ in range(run):
                kl.append(0), sl.append(0), vl.append(0), fl.append(0)
            k, s, v = (ln if field == f else 5 for f in ("key", "subset", "value"))
            kl.append(k), sl.append(s), vl.append(v), fl.append(F_SUBSET | F_VALUE)
            placed[len(kl) - 1] = field
            rows[len(kl) - 1] = (field, ln)
    for _ in range(run):
        kl.append(0), sl.append(0), vl.append(0), fl.append(0)
    c = build(kl, sl, vl, fl, 9, pad=pads_for(kl, sl, vl, placed, mis), seed=7)
    c.rows = {"wave": rows}
    return c


# ---- running a case on the device ---------------------------------------------------------------

GUARD = 0xA5


def to_device(case, dev):
    """The case's columns and heap as torch tensors (int64 offsets and numbers, int32 lengths)."""
    import torch
    ct = {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else
                              (v.view(np.int32) if v.dtype == np.uint32 else v)).to(dev)
          for k, v in case.cols.items()}
    return ct, torch.from_numpy(case.heap).to(dev)


def run_encode(ctx, ct, ht, n, W, shift, cap=None, heap_bytes=None, tail=48):
    """ctx.encode_device into buf[16 + shift:] of a buffer of 16 + shift + W + tail bytes filled with
    GUARD (cap: W + 32 unless given). Returns the wire, frame_off[0..n] and the guard bytes before and
    after the wire, all on the device."""
    import torch
    dev = ht.device
    buf = torch.full((16 + shift + W + tail,), GUARD, dtype=torch.uint8, device=dev)
    foff = torch.full((n + 1,), -7, dtype=torch.int64, device=dev)
    heap = ht if heap_bytes is None else ht[:heap_bytes]
    ctx.encode_device(ct, heap, n, foff, buf[16 + shift:], W + 32 if cap is None else cap)
    torch.cuda.synchronize(dev)
    at = 16 + shift
    return buf[at:at + W], foff, (buf[:at], buf[at + W:])


def first_diff(got_t, exp_t):
    """(index, got, expected) of the first differing byte of two device tensors, or None."""
    ne = (got_t != exp_t).nonzero()
    if ne.numel() == 0:
        return None
    i = int(ne[0])
    return i, int(got_t[i]), int(exp_t[i])


class DevCase:
    """A case on the device with its expected wire and frame offsets there: check(ctx, shift) encodes
    at that output alignment and compares wire, frame_off and guard bytes without a host copy."""

    def __init__(self, case, dev):
        import torch
        self.case, self.n, self.W = case, case.n, len(case.exp)
        self.ct, self.ht = to_device(case, dev)
        self.exp_t = torch.from_numpy(np.frombuffer(case.exp, np.uint8).copy()).to(dev)
        self.foff_t = torch.from_numpy(case.frame_off.view(np.int64)).to(dev)

    def check(self, ctx, shift, cap=None, label=""):
        wire, foff, (head, tail) = run_encode(ctx, self.ct, self.ht, self.n, self.W, shift, cap)
        assert int(foff[self.n]) == self.W, (label, shift, int(foff[self.n]), self.W)
        assert bool((foff == self.foff_t).all()), (label, shift, "frame_off", first_diff(foff, self.foff_t))
        if not bool((wire == self.exp_t).all()):
            i, g, e = first_diff(wire, self.exp_t)
            row = int(np.searchsorted(self.case.frame_off, i, side="right")) - 1
            raise AssertionError(f"{label} shift {shift}: wire byte {i} is {g:#04x}, expected {e:#04x} "
                                 f"(row {row}, byte {i - int(self.case.frame_off[row])} of its frame)")
        assert bool((head == GUARD).all()) and bool((tail == GUARD).all()), (label, shift, "guard bytes")
        return wire
