"""What the claims kernels must predict, worked out from the bytes alone (CPU only).

The speculative decode (csrc/drp_decode_spec.hip, csrc/drp_walk.hip) predicts every tile's claim
and per-thread entry records, and verification repairs whatever was predicted wrongly, so a wrong
prediction never shows in the rows. This module holds the other side of a direct comparison:

  * stream builders: frames at chosen byte positions with whole frames in between (quiet=True:
    payload bytes 0x55 and numbers >= 3, so that the only live positions are the frames' own
    headers and the inner bytes of their multi-byte length varints);
  * the exact model: the chain the exact walk visits from each stream's entry, cut into tile_geo's
    tiles and 64-byte thread segments (claim, entry offset, frames and Change frames per thread);
  * quiet() / decidable(): when the documented prediction rules make the model's values a
    consequence of the bytes, each rule with the kernel line or DESIGN.md paragraph it restates.
    Nothing is excluded by tile number or because a GPU disagreed;
  * the reader of DRP_DUMP_CLAIMS files (drp_launch_spec_head) and the comparator.

tests/test_claims_cases.py checks all of this without a GPU; tests/test_gpu_claims_exact.py holds
the kernels' dump against the model."""
import random
import struct

import numpy as np

import _streams as S

# drp_spec.h / drp_decode_spec.hip
NT, SEGB = 128, 64
TILE = NT * SEGB
HALO = 512
IMG = TILE + HALO
FCAP = 512
KSTRONG = 4
RDY, C_ID, MARK_TERM, M_ERR = 1 << 63, 1 << 62, 1 << 61, 1 << 60
POS_MASK = (1 << 60) - 1
# drp_walk.hip
SY_GENERAL = 2048

H_VALID, H_TAIL_HDR, H_TAIL_CHANGE, H_TAIL_BLOB, H_ERR_VARINT, H_ERR_TYPE, H_ERR_LEN = range(7)


# ---- stream construction: frames at chosen byte positions, valid frames in between -------------
_C2 = S.c2_stream(4096, seed=5).reshape(-1, 86)


def quiet_change(key, i, vlen):
    """A Change whose bytes hold no live position: numbers >= 3 (a byte <= 2 behind a tag byte
    would be one), value bytes 0x55."""
    return S.frame(S.change_payload(key, i % 100 + 3, i % 125 + 3, (i + 1) % 125 + 3, value=b"\x55" * vlen))


def sized_change(n):
    """A quiet Change frame of exactly n bytes (n >= 15), or None where no value length gives it
    (a varint growing by a byte skips a size; a key one byte longer fills that in)."""
    for key in (b"qqq", b"qqqq"):
        base = len(S.frame(S.change_payload(key, 85, 86, 87, value=b"")))
        for vlen in range(max(0, n - base - 4), max(0, n - base) + 1):
            f = S.frame(S.change_payload(key, 85, 86, 87, value=b"\x55" * vlen))
            if len(f) == n:
                return f
    return None


def filler(gap, rng, quiet=False, shaped=False):
    """Exactly `gap` bytes (0 or >= 2) of whole frames: C2 frames, then one or two blobs. quiet:
    payload bytes 0x55 only (no live position but the frames' own headers). shaped (with quiet):
    Change frames only, the last one sized to end the gap, so that every tile's first chain position
    is a Change in the schema's shape (the hop walkers' entry, walk_sync); a gap under 15 bytes is
    one small blob."""
    out = []
    if shaped and gap >= 15:
        assert quiet
        std = S.frame(S.change_payload(b"qqq", 85, 86, 87, value=b"\x55" * 70))
        while gap >= 300:
            out.append(std)
            gap -= len(std)
        for first in range(gap, 14, -1):  # one sized Change, or two where a size is skipped
            a, b = sized_change(first), (sized_change(gap - first) if gap - first else b"")
            if a is not None and b is not None and (gap == first or gap - first >= 15):
                out += [a, b]
                return b"".join(out)
        raise AssertionError("no Changes of %d bytes" % gap)
    while gap >= 300:
        if quiet:
            out.append(S.frame(S.change_payload(b"qqq", 85, 86, 87, value=b"\x55" * 70)))
        else:
            out.append(_C2[rng.randrange(len(_C2))].tobytes())
        gap -= len(out[-1])
    if gap == 129:
        out.append(S.frame(b"\x55" * 62 if quiet else bytes(62), 2))
        gap -= 64
    if gap:
        assert gap >= 2, gap
        n = gap - 2 if gap <= 128 else gap - 3
        out.append(S.frame(b"\x55" * n if quiet else rng.randbytes(n), 2))
        assert len(out[-1]) == gap, (len(out[-1]), gap)
    return b"".join(out)


def place(items, rng, end=None, quiet=False, shaped=False):
    """A stream with frame bytes items[i][1] starting at position items[i][0] (ascending)."""
    w = bytearray()
    for pos, fr in items:
        w += filler(pos - len(w), rng, quiet, shaped)
        w += fr
    if end is not None:
        w += filler(end - len(w), rng, quiet, shaped)
    return bytes(w)


def header_frame(k, i, quiet=False):
    """A Change frame whose length varint takes k bytes."""
    vlen = {1: 40, 2: 300, 3: 17000}[k]
    if quiet:
        f = quiet_change(b"k%06d" % i, i, vlen)
    else:
        f = S.frame(S.change_payload(b"k%06d" % i, i % 100 + 1, i % 128, (i + 1) % 128,
                                     value=(bytes(range(7, 256)) * (vlen // 249 + 1))[:vlen]))
    assert f[k - 1] < 0x80 and all(b >= 0x80 for b in f[:k - 1])
    return f


def straddle_cases():
    """(k, j, e) in stream order, and the (stream, tile) each lands in: a header of a k-byte length
    varint starts j bytes before offset e of its tile's halo (e = 0: the tile end)."""
    rng = random.Random(41)
    cases = [(k, j, e) for k in (1, 2, 3) for j in range(1, k + 1) for e in range(0, HALO + 1, 16)]
    rng.shuffle(cases)
    return rng, cases


def straddle_streams(quiet=False, where=None, shaped=False):
    """Headers of 1-, 2- and 3-byte length varints (+ the id byte) that begin j = 1..k bytes before
    the tile end and before every 16-byte edge of the halo (the image's end included): one case
    per tile (three tiles for the 16 KB frames), streams of at most 40 tiles. where: a list that
    receives (stream, tile, k, j, e) per case (the header starts at tile * TILE + e - j). shaped:
    filler()'s form without blobs."""
    rng, cases = straddle_cases()
    streams, items, t = [], [], 1
    for i, (k, j, e) in enumerate(cases):
        items.append((t * TILE + e - j, header_frame(k, i, quiet)))
        if where is not None:
            where.append((len(streams), t, k, j, e))
        t += 4 if k == 3 else 1
        if t > 36:
            streams.append(place(items, rng, end=t * TILE + 1000, quiet=quiet, shaped=shaped))
            items, t = [], 1
    if items:
        streams.append(place(items, rng, end=t * TILE + 1000, quiet=quiet, shaped=shaped))
    return streams


def live_mask(wire, lo, hi):
    """Live positions in [lo, hi): a varint of 1..3 bytes, then a byte <= 2 (the claims' listing
    rule, drp_decode_spec.hip "live = X0 | (M0 & (Xs1 | (Ms1 & Xs2)))"); bytes past the wire read
    as 0x55."""
    b = np.frombuffer(wire[lo:hi + 4], np.uint8).astype(np.int64)
    b = np.pad(b, (0, max(0, hi + 4 - lo - len(b))), constant_values=0x55)
    m, s = b >= 0x80, b <= 2
    x = ~m[:-1] & s[1:]
    n = hi - lo
    return x[:n] | (m[:n] & x[1:n + 1]) | (m[:n] & m[1:n + 1] & x[2:n + 2])


def live_count(wire, lo, hi):
    return int(live_mask(wire, lo, hi).sum())


# ---- the families of tests/test_gpu_claims_exact.py ----------------------------------------------
# Every builder returns a list of cases: dicts with "wire", "stream_off" (n + 1 offsets), "entry"
# (n offsets), "named": the (stream, tile) pairs the case is named for, and "forms": the claims forms
# it is named for ("fast": claims_fast / spec_claims, "hop": the hop walkers).
FORMS = ("fast", "hop")


def _single(wire, named=(), forms=FORMS):
    return {"wire": wire, "stream_off": [0, len(wire)], "entry": [0], "named": [(0, t) for t in named],
            "forms": forms}


def family_a():
    """The quiet straddle streams."""
    where = []
    streams = straddle_streams(quiet=True, where=where, shaped=True)
    # (a case is named for the tile whose end / halo the header straddles, tile - 1, and for the
    # tile the header's frame ends in or passes)
    return [_single(w, sorted({t - 1 for s, t, k, j, e in where if s == i} | {t for s, t, k, j, e in where if s == i}))
            for i, w in enumerate(streams)]


def image_end_items():
    return [((d + 1) * TILE + HALO - d, quiet_change(b"%010d" % d, d, 64)) for d in range(1, 20)]


def family_b():
    """A frame starts in each of the image's last 19 bytes (the last 16 are never listed, the three
    before them have their lookahead there)."""
    rng = random.Random(47)
    return [_single(place(image_end_items(), rng, end=21 * TILE + 300, quiet=True, shaped=True), range(1, 21))]


C_RUNS = ((67, 3), (133, 5))  # (frame bytes, tiles): 1- and 2-byte length varints, both coprime to 64


def family_c():
    """Runs of equal quiet Change frames whose length is coprime to 64: carriers at every entry
    offset and in every thread, headers across a thread edge included."""
    w = bytearray(filler(TILE - 30, random.Random(59), quiet=True, shaped=True))
    i = 0
    for flen, tiles in C_RUNS:
        stop = len(w) + tiles * TILE
        vl = next(v for v in range(flen) if len(quiet_change(b"c%05d" % 0, 0, v)) == flen)
        while len(w) < stop:
            f = quiet_change(b"c%05d" % i, i, vl)
            assert len(f) == flen, (len(f), flen)
            w += f
            i += 1
    w += filler(700, random.Random(61), quiet=True, shaped=True)
    return [_single(bytes(w), range(1, len(w) // TILE))]


def _run_stream(unit, run_bytes, seed):
    """A quiet tile, a run of `unit` of about run_bytes bytes, and quiet frames to past an image.
    The run's length is the first (in whole units, downwards) at which the stream is quiet: the run's
    last shadows land in the frames behind it."""
    rng0 = random.Random(seed)
    head = filler(TILE + 1000, rng0, quiet=True, shaped=True)
    for n in range(run_bytes // len(unit), run_bytes // len(unit) - 64, -1):
        rng = random.Random(seed + 1)
        body = head + unit * n
        w = body + filler((len(body) // TILE + 3) * TILE + 700 - len(body), rng, quiet=True, shaped=True)
        if quiet(StreamModel(w, 0, len(w), 0))[0]:
            return w
    raise AssertionError("no quiet run length")


SEED8 = b"\x05\x01" + b"\x55" * 6  # a live position that parses as one frame and lands on an error header


def capacity_stream(total_want):
    """Three quiet tiles; tile 1 holds a blob whose payload is seeded with dead live positions
    (SEED8) so that tile 1 and its halo list exactly total_want positions."""
    for seeds in range(total_want, 0, -1):
        pay = SEED8 * seeds + b"\x55" * (6000 - 8 * seeds)
        # (a Change starts the tile: the hop walkers' entry; the blob follows it)
        w = place([(TILE + 10, quiet_change(b"cap", 1, 40)), (TILE + 200, S.frame(pay, 2))], random.Random(43),
                  end=3 * TILE + 900, quiet=True, shaped=True)
        if live_count(w, TILE, TILE + IMG - 16) == total_want:
            return w
    raise AssertionError("no seed count gives %d live positions" % total_want)


def family_d():
    """Dense and empty threads: runs of 3-byte blob frames (21-22 frames per thread) and of id-0
    headers (carriers that deliver nothing), both past FCAP live positions per tile, and a tile at
    exactly FCAP and FCAP + 1 live positions."""
    blobs = _run_stream(b"\x02\x02\x55", 2 * TILE + 4000, 67)
    zeros = _run_stream(b"\x55\x00", 2 * TILE + 4000, 71)
    # (the runs hold no shaped Change, the hop walkers' only sync: named for the fast form alone)
    return [_single(blobs, (2, 3), ("fast",)), _single(zeros, (2, 3), ("fast",)),
            _single(capacity_stream(FCAP), (1,)), _single(capacity_stream(FCAP + 1), (1,))]


def family_e():
    """Long frames: a 17000-byte Change and a three-tile blob (identity tiles), 4 KB Changes that
    start in a tile and in a halo (strong by structure with DRP_CHANGE_CHECKS=1, through the
    deferred check without), and a blob that leaves the image."""
    rng = random.Random(73)
    items = [(TILE + 3000, quiet_change(b"long", 1, 17000)),
             (5 * TILE - 40, S.frame(b"\x55" * (3 * TILE + 500), 2))]
    pos = 9 * TILE + 6000
    for i in range(6):  # 4 KB values from inside tile 9: the later ones start in tiles and in halos
        items.append((pos, quiet_change(b"v%05d" % i, i, 4096)))
        pos += len(items[-1][1])
    items.append((13 * TILE + 100, quiet_change(b"halo", 7, 4096)))      # starts in tile 12's halo
    items.append((15 * TILE - 700, S.frame(b"\x55" * 12000, 2)))          # a blob that leaves the image
    w = place(items, rng, end=19 * TILE + 800, quiet=True, shaped=True)
    return [_single(w, (1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15, 16))]


def family_f():
    """Edges: three streams at unaligned offsets in one call. The first starts inside a blob (a
    non-zero entry) and ends in a cut header, the second ends in a cut Change, the third in a cut
    blob; every tail has more than KSTRONG whole frames before it in its tile."""
    def body(seed, n):
        return filler(n, random.Random(seed), quiet=True, shaped=True)
    s0 = b"\x55" * 777 + body(79, 2 * TILE + 3000) + quiet_change(b"cut", 3, 300)[:1]
    s1 = body(83, 3 * TILE + 2500) + quiet_change(b"cutc", 4, 300)[:150]
    s2 = body(89, 2 * TILE + 5000) + S.frame(b"\x55" * 500, 2)[:200]
    # (stream_off is one ascending list: the bytes between the three are short streams of whole
    # quiet frames, compared like the others)
    parts = [body(103, 3000), s0, body(107, 1234), s1, body(109, 4321), s2]
    so = [0]
    for p in parts:
        so.append(so[-1] + len(p))
    named = []
    for s in (1, 3, 5):
        nt = (((so[s + 1] + TILE - 1) & ~(TILE - 1)) - (so[s] & ~(TILE - 1))) // TILE
        named += [(s, 0), (s, nt - 1)]
    return [{"wire": b"".join(parts), "stream_off": so, "entry": [0, 777, 0, 0, 0, 0], "named": named,
             "forms": FORMS}]


def family_g():
    """Dead shadows: every frame's value ends in SEED8, ten bytes before the next real header, so a
    seeded candidate lies before the real header in the same 64-byte segment; the thread's first
    strong node must be the real one."""
    w = bytearray(filler(TILE - 30, random.Random(97), quiet=True, shaped=True))
    i = 0
    while len(w) < 4 * TILE:
        f = S.frame(S.change_payload(b"g%05d" % i, i % 100 + 3, 4, 5, value=b"\x55" * 41 + SEED8 + b"\x55\x55"))
        w += f
        i += 1
    w += filler(700, random.Random(101), quiet=True, shaped=True)
    return [_single(bytes(w), (1, 2, 3))]


FAMILIES = {"A": family_a, "B": family_b, "C": family_c, "D": family_d, "E": family_e, "F": family_f,
            "G": family_g}
_cache = {}


def family(name):
    """The cases of a family with their models, built once."""
    if name not in _cache:
        cases = FAMILIES[name]()
        for c in cases:
            c["model"] = BatchModel(c["wire"], c["stream_off"], c["entry"])
        _cache[name] = cases
    return _cache[name]


# ---- the exact model -------------------------------------------------------------------------------
def parse_hdr(w, p, se):
    """parse_win (drp_spec.h) at absolute position p of a stream that ends at se:
    (kind, id, varint bytes, L, successor)."""
    avail = se - p
    L, k = 0, 0
    for i in range(10):
        if i >= avail:
            return H_TAIL_HDR, 0, 0, L, 0
        b = w[p + i]
        if i == 9 and (b & 0x7F) > 1:
            return (H_TAIL_HDR if avail < 11 else H_ERR_VARINT), 0, 0, L, 0
        L |= (b & 0x7F) << (7 * i)
        if not b & 0x80:
            k = i + 1
            break
    else:
        return (H_TAIL_HDR if avail < 11 else H_ERR_VARINT), 0, 0, L, 0
    if k >= avail:
        return H_TAIL_HDR, 0, k, L, 0
    fid = w[p + k]
    if fid >= 3:
        return H_ERR_TYPE, fid, k, L, 0
    if fid == 0:
        return H_VALID, 0, k, L, p + k + 1
    if L == 0:
        return H_ERR_LEN, fid, k, L, 0
    if L > avail - k:
        return (H_TAIL_CHANGE if fid == 1 else H_TAIL_BLOB), fid, k, L, 0
    return H_VALID, fid, k, L, p + k + L


class StreamModel:
    """The exact chain of one stream: pos (every header the walk visits from the entry, id-0 headers
    and the tail or error header included), what each delivers, and how the chain ends."""

    def __init__(self, wire, so, se, entry):
        self.wire, self.so, self.se, self.e0 = wire, so, se, so + entry
        self.base = so & ~(TILE - 1)
        self.ntiles = (((se + TILE - 1) & ~(TILE - 1)) - self.base) // TILE if se > so else 0  # tile_prefix_body
        pos, deliv, chg, whole = [], [], [], []
        p, self.end, self.err = self.e0, "end", 0
        while p < se:
            kind, fid, k, L, succ = parse_hdr(wire, p, se)
            pos.append(p)
            deliv.append((kind == H_VALID and fid != 0) or kind == H_TAIL_BLOB)  # hdr_delivered (drp_device.h)
            chg.append(kind == H_VALID and fid == 1)
            whole.append(kind == H_VALID)
            if kind != H_VALID:
                self.end = "tail" if kind <= H_TAIL_BLOB else "error"
                self.err = kind
                break
            p = succ
        self.pos = np.array(pos, np.int64)
        self.deliv, self.chg, self.whole = np.array(deliv, bool), np.array(chg, bool), np.array(whole, bool)
        self.chainset = set(pos)
        self.nframes, self.nchanges = int(self.deliv.sum()), int(self.chg.sum())
        self._quiet = None

    def tile_range(self, t):
        a = self.base + t * TILE
        return a, int(np.searchsorted(self.pos, a)), int(np.searchsorted(self.pos, a + TILE))

    def claim(self, t):
        """None (identity: no chain position in the tile), or (exit, term): the first chain position
        >= the tile's end, the stream end when the chain ends there, or (term) the tail's position
        when the chain ends in a tail inside the tile (walk(), drp_decode_spec.hip:108-125)."""
        a, i, j = self.tile_range(t)
        if i == j:
            return None
        if j < len(self.pos):
            return int(self.pos[j]), False
        if self.end == "end":
            return self.se, False
        return int(self.pos[-1]), True

    def records(self, t):
        """(ent, n, c) of the tile's NT threads: the offset of the first chain position in the
        thread's 64 bytes (-1: none), and the delivered frames / Change frames whose header the chain
        visits from there before the segment's end."""
        a, i, j = self.tile_range(t)
        ent = np.full(NT, -1, np.int64)
        rel = self.pos[i:j] - a
        th = rel // SEGB
        n = np.bincount(th, weights=self.deliv[i:j], minlength=NT).astype(np.int64)
        c = np.bincount(th, weights=self.chg[i:j], minlength=NT).astype(np.int64)
        first = np.ones(len(th), bool)
        first[1:] = th[1:] != th[:-1]
        ent[th[first]] = rel[first] % SEGB
        return ent, n, c


class BatchModel:
    def __init__(self, wire, stream_off, entry):
        self.wire = wire
        self.streams = [StreamModel(wire, stream_off[s], stream_off[s + 1], entry[s]) for s in range(len(entry))]
        self.first = np.concatenate([[0], np.cumsum([m.ntiles for m in self.streams])]).astype(np.int64)
        self.ntiles = int(self.first[-1])

    def tiles(self):
        """(global tile, stream, tile of the stream) in the dump's order."""
        for s, m in enumerate(self.streams):
            for t in range(m.ntiles):
                yield int(self.first[s]) + t, s, t


# ---- quietness and decidability ------------------------------------------------------------------
def follow(m, q):
    """The candidate chain from live position q through parse_win's grammar: (frames, how): how is
    "dies" (an error header, or a tail: strong() drops a tail within three frames of a candidate,
    drp_decode_spec.hip:158-160, and claims_fast's parse leaves a tail node dead), "lands" (it
    reaches a chain position or the stream end) or "survives" (KSTRONG whole frames)."""
    chain = m.chainset
    p, frames = q, 0
    while frames < KSTRONG:
        kind, fid, k, L, succ = parse_hdr(m.wire, p, m.se)
        if kind != H_VALID:
            return frames, "dies"
        frames += 1
        p = succ
        if p in chain or p >= m.se:
            return frames, "lands"
    return frames, "survives"


def shadows(m):
    """Every live position of the stream that is not a chain position, with follow()'s verdict."""
    live = np.flatnonzero(live_mask(m.wire, m.so, m.se)) + m.so
    return [(int(q),) + follow(m, int(q)) for q in live if int(q) not in m.chainset]


def quiet(m):
    """(is quiet, shadows): every live position that is not a chain position dies before KSTRONG
    frames and never lands on a chain position (DESIGN.md "Why predictions hold": "positions that
    parse as a header ... die within a frame ...; the stream's own chain never dies"; the survival
    rounds, drp_decode_spec.hip "survival: KSTRONG - 1 rounds")."""
    if m._quiet is None:
        sh = shadows(m)
        m._quiet = (all(how == "dies" for _, _, how in sh), sh)
    return m._quiet


def _uvarint(w, p, lim=10):
    v = 0
    for i in range(lim):
        b = w[p + i] if p + i < len(w) else 0
        v |= (b & 0x7F) << (7 * i)
        if not b & 0x80:
            return i + 1, v
    return 0, 0


def change_shape(w, po, pl):
    """wk_change_shape (drp_walk.hip:180-219): the payload parses in the schema's own field order
    ([subset] key change from to [value]) and its last field ends the payload."""
    off, last = 0, 0
    for _ in range(6):
        if off >= pl:
            break
        b0 = w[po + off] if po + off < len(w) else 0
        fn, wt = b0 >> 3, b0 & 7
        if b0 >= 0x80 or fn < 1 or fn > 6 or fn <= last:
            return False
        num = 3 <= fn <= 5
        if wt != (0 if num else 2):
            return False
        if (fn == 3 and last < 2) or (fn > 3 and last != fn - 1):
            return False
        kb, v = _uvarint(w, po + off + 1)
        if kb == 0 or (kb > 5 and not num) or 1 + kb > pl - off:
            return False
        off += 1 + kb
        if not num:
            if v > pl - off:
                return False
            off += v
        last = fn
    return off == pl and last >= 5


def shaped(w, c, se):
    """wk_shaped (drp_walk.hip:223-233): a complete Change at c in the schema's shape whose next
    header is valid."""
    if c >= se:
        return False
    k, L = _uvarint(w, c, 5)
    if k == 0 or c + k >= len(w) or w[c + k] != 1 or L <= 1 or L - 1 > se - c - k - 1:
        return False
    if not change_shape(w, c + k + 1, L - 1):
        return False
    n = c + k + L
    if n >= se:
        return True
    k2, L2 = _uvarint(w, n, 5)
    if k2 == 0 or n + k2 >= len(w):
        return False
    fid = w[n + k2]
    return fid <= 2 and (fid == 0 or L2 != 0)


def first_shaped(m, a):
    """walk_sync's shaped scan over tile [a, a + TILE) (sync_entry, drp_walk.hip:496-528): the first
    position with a 1..3-byte length varint, the id 1 and the tag 0x0a / 0x12 (wk_shape16) that
    passes wk_shaped."""
    w = m.wire
    live = np.flatnonzero(live_mask(w, a, a + TILE)) + a
    for q in live.tolist():
        k, _ = _uvarint(w, q, 3)
        if k and q + k + 1 < len(w) and w[q + k] == 1 and w[q + k + 1] in (0x0A, 0x12) and shaped(w, q, m.se):
            return q
    return None


def interior(m, t):
    """claims_fast's / walk_regions' interior tiles: the image [A, A + IMG) lies inside the stream
    (claims_fast: "G.A < G.so || G.A + IMG > G.se" is an edge tile; interior(), drp_walk.hip:53-66)."""
    a = m.base + t * TILE
    return a >= m.so and a + IMG <= m.se


def decidable(m, t, form):
    """(decidable, first thread whose records are compared, reason). form: "fast" (claims_fast and
    spec_claims) or "hop" (the hop walkers; their edge tiles are spec_claims')."""
    if m.end == "error":  # (the claims past an error are predictions the exact walk corrects: tests/test_gpu_walk.py)
        return False, 0, "the chain ends in an error"
    if not quiet(m)[0]:
        return False, 0, "not quiet"
    a, i, j = m.tile_range(t)
    if form == "hop" and interior(m, t):
        if a == m.so:
            # a stream's first tile has its exact entry (sync_entry: "if (G.exact) return G.entry")
            return True, int((m.pos[i] - a) // SEGB) if i < j else 0, "exact entry"
        if i == j:
            # no shaped candidate: the general scan takes only candidates that pass wk_survives
            # (sync_general, drp_walk.hip:365-394), which needs WK_K = 8 whole frames, or at least two
            # before the stream end or a tail (drp_walk.hip:243-269); a candidate that dies within one
            # frame passes neither, and then the region has no entry: identity
            cand = np.flatnonzero(live_mask(m.wire, a, a + SY_GENERAL)) + a
            if first_shaped(m, a) is None and all(follow(m, int(q)) in ((0, "dies"), (1, "dies")) for q in cand):
                return True, 0, "no candidate of the general scan survives a second frame"
            return False, 0, "the general scan has candidates"
        # walk_sync's rule: the region's entry is its first shaped Change (DESIGN.md "Sync"); an
        # earlier candidate is taken only when its chain lands exactly on it (sync_merges), which a
        # quiet stream has none of
        p0 = int(m.pos[i])
        if first_shaped(m, a) == p0:
            return True, (p0 - a) // SEGB, "first chain position is the first shaped Change"
        return False, 0, "first chain position is no shaped Change"
    if i == j:
        # no strong candidate, and every deferred one dies in HBM: identity (DESIGN.md "(or
        # 'identity' when no chain survives: the tile sits inside a long payload)")
        return True, 0, "no chain position"
    # a chain too short to be strong before its tail is left unclaimed (DESIGN.md "Repair"); the list
    # form needs KSTRONG whole frames from the candidate (drp_decode_spec.hip "survival" rounds), or a
    # chain that ends at the stream end ("ends at the stream end: survived", NX_NEAR; strong():
    # "reached the stream end: survived")
    whole = int(m.whole[i:].sum())
    if whole >= KSTRONG or m.end == "end":
        return True, 0, "strong first chain position"
    return False, 0, "fewer than KSTRONG frames before the tail"


# ---- the dump ------------------------------------------------------------------------------------
def read_dump(path):
    """DRP_DUMP_CLAIMS (drp_launch_spec_head): blocks of u64 ntl, ntl claim words, ntl * 128 bytes
    each of ent, ent_n, ent_c."""
    data = open(path, "rb").read()
    blocks, o = [], 0
    while o < len(data):
        (ntl,) = struct.unpack_from("<Q", data, o)
        o += 8
        need = ntl * 8 + 3 * ntl * NT
        assert o + need <= len(data), "truncated dump block"
        cl = np.frombuffer(data, "<u8", ntl, o)
        o += ntl * 8
        rec = np.frombuffer(data, np.uint8, 3 * ntl * NT, o).reshape(3, ntl, NT)
        o += 3 * ntl * NT
        blocks.append({"ntl": ntl, "claim": cl, "ent": rec[0], "ent_n": rec[1], "ent_c": rec[2]})
    return blocks


def write_dump(path, model, mode="wb"):
    """The model's own values in the dump's format (tests of the comparator)."""
    ntl = model.ntiles
    cl = np.zeros(ntl, "<u8")
    rec = np.zeros((3, ntl, NT), np.uint8)
    for g, s, t in model.tiles():
        m = model.streams[s]
        c = m.claim(t)
        cl[g] = RDY | (C_ID if c is None else (c[0] | (MARK_TERM if c[1] else 0)))
        ent, n, ch = m.records(t)
        rec[0, g] = np.where(ent < 0, 0xFF, ent).astype(np.uint8)
        rec[1, g], rec[2, g] = n, ch
    with open(path, mode) as f:
        f.write(struct.pack("<Q", ntl))
        f.write(cl.tobytes())
        f.write(rec.tobytes())


def compare(block, model, form):
    """Mismatches (tile, thread, field, got, want) between a dump block and the model on every
    decidable tile (thread -1: the tile's claim word)."""
    out = []
    if block["ntl"] != model.ntiles:
        return [(-1, -1, "ntl", int(block["ntl"]), model.ntiles)]
    for g, s, t in model.tiles():
        m = model.streams[s]
        ok, th0, _ = decidable(m, t, form)
        if not ok:
            continue
        got = int(block["claim"][g]) & ~RDY
        want = m.claim(t)
        if want is None:
            if not got & C_ID:
                out.append((g, -1, "claim", hex(got), "identity"))
        elif got & C_ID:
            out.append((g, -1, "claim", "identity", want[0]))
        else:
            if got & POS_MASK != want[0]:
                out.append((g, -1, "claim", got & POS_MASK, want[0]))
            if bool(got & MARK_TERM) != want[1]:
                out.append((g, -1, "term", bool(got & MARK_TERM), want[1]))
        ent, n, c = m.records(t)
        ge, gn, gc = block["ent"][g], block["ent_n"][g], block["ent_c"][g]
        seen = False  # a carrier before this thread (in the dump)
        for th in range(th0, NT):
            e = int(ge[th])
            if ent[th] < 0:
                if e != 0xFF:
                    out.append((g, th, "ent", e, 0xFF))
            elif e == 0xFF or (e & 0x3F) != ent[th] or e & 0x80:
                out.append((g, th, "ent", e, int(ent[th])))
            if e != 0xFF:
                # verify_lite: "no later thread may restart the chain" (restart_bytes)
                if seen and e & 0x40:
                    out.append((g, th, "restart", e, e & 0x3F))
                seen = True
            if int(gn[th]) != n[th]:
                out.append((g, th, "ent_n", int(gn[th]), int(n[th])))
            if int(gc[th]) != c[th]:
                out.append((g, th, "ent_c", int(gc[th]), int(c[th])))
    return out
