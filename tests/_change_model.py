"""An independent model of the Change payload decode, and the matrix of payloads that walks it.

The model restates the decode from the policy text ("Policy for inputs the reference
leaves undefined") and the comment above oracle_change_decode, not from the C: arbitrary-precision
integers, an explicit ToInt32, one varint reader that looks at the whole varint before it judges
it. The oracle (oracle/drp_oracle.c) and the device decoders (csrc/drp_device.h,
csrc/drp_decode_spec.hip) must agree with it bit for bit; tests/test_change_matrix.py holds the
model against the oracle, tests/test_gpu_change_matrix.py holds the kernels against both.

The rules, as the policy states them:
  * a payload is a sequence of fields, each a varint prefix then a body; tag = ToInt32(prefix) >> 3
    (arithmetic), wire = prefix & 7;
  * a varint is 7 bits per byte, least significant first, the top bit meaning "more"; one that the
    payload cuts, one longer than 10 bytes or one worth 2^64 or more is malformed;
  * a prefix or a length (where the reference forms a JS Number and uses it as one) of 2^53 or more
    is malformed; change / from / to keep their full 64-bit value;
  * tags 1, 2, 6 (subset, key, value) are a length and that many bytes, tags 3, 4, 5 (change,
    from, to) a varint, whatever wire type the prefix names; a body that runs past the payload is
    malformed;
  * any other tag is skipped by wire type (0 varint, 1 eight bytes, 2 length + bytes, 5 four
    bytes); wire types 3, 4, 6, 7 are malformed;
  * a later field replaces an earlier one of the same tag;
  * malformed is DRP_ERR_CHANGE with DRP_F_BAD, the fields read before it kept; a payload that
    ends without key, change, from or to is DRP_ERR_REQUIRED with DRP_F_BAD | DRP_F_MISSING.
"""
import random

F_SUBSET, F_VALUE, F_BAD, F_MISSING = 1, 2, 4, 8
ERR_NONE, ERR_CHANGE, ERR_REQUIRED = 0, 4, 5

COLS = ["key_off", "key_len", "subset_off", "subset_len", "value_off", "value_len", "change", "from", "to"]
NAMES = {1: "subset", 2: "key", 3: "change", 4: "from", 5: "to", 6: "value"}
REQUIRED = ["key", "change", "from", "to"]


def to_int32(x):
    """ECMAScript ToInt32 of a non-negative integer."""
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x & 0x80000000 else x


class _Bad(Exception):
    pass


def _all_labels():
    out = {"empty", "ok", "tag.wrap", "tag.negative", "tag.ge2p53", "len.ge2p53", "len.past_end", "num.ge2p53",
           "skip.varint", "skip.fixed64", "skip.fixed64.cut", "skip.bytes", "skip.bytes.ge2p53",
           "skip.bytes.past_end", "skip.fixed32", "skip.fixed32.cut", "order.canonical", "order.other"}
    for what in ["tag", "len", "num", "skip.varint", "skip.len"]:
        out |= {f"{what}.cut", f"{what}.long", f"{what}.ge2p64"}
    for what in ["tag", "len", "num"]:
        out |= {f"{what}.w{k}" for k in range(1, 11)} | {f"{what}.padded"}
    out |= {f"skip.wire{w}" for w in (3, 4, 6, 7)}
    out |= {f"known{t}.wire{w}" for t in range(1, 7) for w in range(8)}
    out |= {f"dup.{n}" for n in NAMES.values()} | {f"missing.{n}" for n in REQUIRED}
    return out


LABELS = frozenset(_all_labels())


def decode(p):
    """The model's decode of payload `p` (bytes): a dict of the nine columns, flags, err and
    labels (the set of branch labels the payload passed through)."""
    p = bytes(p)
    n = len(p)
    col = dict.fromkeys(COLS, 0)
    flags, seen, order, labels = 0, set(), [], set()

    def varint(at, what):
        # the whole varint first (up to its terminator or the payload's end), then the verdict
        end = at
        while end < n and p[end] & 0x80:
            end += 1
        width = end - at + 1
        if width > 10:
            labels.add(what + ".long")
            raise _Bad
        if end >= n:
            labels.add(what + ".cut")
            raise _Bad
        v = sum((p[at + i] & 0x7F) << (7 * i) for i in range(width))
        if v >> 64:
            labels.add(what + ".ge2p64")
            raise _Bad
        if what in ("tag", "len", "num"):
            labels.add(f"{what}.w{width}")
            if width > 1 and p[end] == 0:
                labels.add(what + ".padded")
        return v, end + 1

    def length(at, what):
        v, at = varint(at, what)
        if v >= 1 << 53:
            labels.add("len.ge2p53" if what == "len" else "skip.bytes.ge2p53")
            raise _Bad
        if v > n - at:
            labels.add("len.past_end" if what == "len" else "skip.bytes.past_end")
            raise _Bad
        return v, at

    err = ERR_NONE
    if n == 0:
        labels.add("empty")
    try:
        at = 0
        while at < n:
            start = at
            prefix, at = varint(at, "tag")
            if prefix >= 1 << 53:
                labels.add("tag.ge2p53")
                raise _Bad
            t32 = to_int32(prefix)
            if t32 != prefix:
                labels.add("tag.wrap")
            tag, wire = t32 >> 3, prefix & 7
            if tag < 0:
                labels.add("tag.negative")
            if tag in NAMES:
                name = NAMES[tag]
                labels.add(f"known{tag}.wire{wire}")
                if tag in (1, 2, 6):
                    ln, at = length(at, "len")
                    col[name + "_off"], col[name + "_len"] = at, ln
                    at += ln
                    flags |= F_SUBSET if tag == 1 else F_VALUE if tag == 6 else 0
                else:
                    v, at = varint(at, "num")
                    if v >= 1 << 53:
                        labels.add("num.ge2p53")
                    col[name] = v
                if name in seen:
                    labels.add("dup." + name)
                seen.add(name)
                order.append(name)
            elif wire == 0:
                _, at = varint(at, "skip.varint")
                labels.add("skip.varint")
            elif wire == 1:
                if n - at < 8:
                    labels.add("skip.fixed64.cut")
                    raise _Bad
                at += 8
                labels.add("skip.fixed64")
            elif wire == 2:
                ln, at = length(at, "skip.len")
                at += ln
                labels.add("skip.bytes")
            elif wire == 5:
                if n - at < 4:
                    labels.add("skip.fixed32.cut")
                    raise _Bad
                at += 4
                labels.add("skip.fixed32")
            else:
                labels.add(f"skip.wire{wire}")
                raise _Bad
            assert at > start
        missing = [k for k in REQUIRED if k not in seen]
        if missing:
            labels.update("missing." + k for k in missing)
            err, flags = ERR_REQUIRED, flags | F_BAD | F_MISSING
        else:
            labels.add("ok")
            canon = [k for k in ["subset", "key", "change", "from", "to", "value"] if k in seen]
            labels.add("order.canonical" if order == canon else "order.other")
    except _Bad:
        err, flags = ERR_CHANGE, flags | F_BAD
    assert labels <= LABELS, labels - LABELS
    return dict(col, flags=flags, err=err, labels=labels)


# ---- building payloads ----------------------------------------------------------------------------

def vi(v, width=0):
    """varint of v, padded with 0x80 ... 0x00 to `width` bytes when that is longer."""
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    if width > len(out):
        out[-1] |= 0x80
        out += b"\x80" * (width - len(out) - 1) + b"\x00"
    return bytes(out)


def field(tag, body, wire=None, width=0):
    """One field: the prefix of `tag` (its natural wire type unless given), then for a bytes body
    its length and the bytes, for an int body its varint."""
    if wire is None:
        wire = 2 if isinstance(body, (bytes, bytearray)) else 0
    pre = vi((tag << 3) | wire, width)
    if isinstance(body, (bytes, bytearray)):
        return pre + vi(len(body)) + bytes(body)
    return pre + vi(body)


KEY, SUBSET, VALUE = b"k1", b"su", b"value!"
CANON = {"subset": None, "key": KEY, "change": 5, "from": 6, "to": 7, "value": VALUE}
TAG = {v: k for k, v in NAMES.items()}


def fields(order=("subset", "key", "change", "from", "to", "value"), **over):
    f = dict(CANON, **over)
    return b"".join(field(TAG[k], f[k]) for k in order if f[k] is not None)


class Entry:
    """A named payload; marks = payload offsets inside a varint worth putting a tile edge in."""

    def __init__(self, name, payload, marks=()):
        self.name, self.payload, self.marks = name, bytes(payload), tuple(marks)

    def __repr__(self):
        return f"Entry({self.name!r}, {len(self.payload)} B)"


def change_matrix():
    """The named payloads: at least one per branch label of the model (test_change_matrix.py
    checks that the union of their labels is the full set)."""
    m = []
    add = lambda name, payload, marks=(): m.append(Entry(name, payload, marks))
    rest = field(3, 5) + field(4, 6) + field(5, 7)  # change, from, to behind a key
    full = fields()

    add("canonical", full)
    add("canonical.subset", fields(subset=SUBSET))
    add("canonical.no_value", fields(value=None))
    add("canonical.empty_strings", fields(subset=b"", key=b"", value=b""))
    add("empty", b"")
    add("only.subset", field(1, SUBSET))
    add("only.value", field(6, VALUE))
    for k in REQUIRED:
        add(f"missing.{k}", fields(**{k: None}))
    add("reversed", fields(order=("value", "to", "from", "change", "key", "subset"), subset=SUBSET))
    for k in NAMES.values():
        other = {"subset": b"S2", "key": b"other-key", "change": 300, "from": 1 << 40, "to": 0, "value": b""}[k]
        add(f"dup.{k}", fields(subset=SUBSET) + field(TAG[k], other))
        add(f"dup.{k}.first", field(TAG[k], other) + fields(subset=SUBSET))

    # every varint width, for the tag, a length and a number: padded (0x80 ... 0x00) and, for
    # numbers, natural
    for w in range(1, 11):
        add(f"tag.w{w}", vi(0x12, w) + vi(len(KEY)) + KEY + rest, marks=(1,) if w > 1 else ())
        add(f"len.w{w}", b"\x12" + vi(len(KEY), w) + KEY + rest, marks=(2,) if w > 1 else ())
        add(f"num.pad{w}", field(2, KEY) + b"\x18" + vi(5, w) + field(4, 6) + field(5, 7),
            marks=(len(field(2, KEY)) + 2,) if w > 1 else ())
        v = 1 if w == 1 else 1 << (7 * (w - 1))
        add(f"num.w{w}", field(2, KEY) + field(3, v) + field(4, v + 1 if w < 10 else v) + field(5, 7),
            marks=(len(field(2, KEY)) + 2,) if w > 1 else ())
        # a value's length and an unknown field's, padded too
        add(f"value.len.w{w}", field(2, KEY) + rest + b"\x32" + vi(len(VALUE), w) + VALUE)
        add(f"unknown.len.w{w}", field(2, KEY) + b"\x7a" + vi(3, w) + b"abc" + rest)
        add(f"unknown.varint.w{w}", field(2, KEY) + b"\x78" + vi(9, w) + rest)
    # a wide prefix in front of a ten-byte varint: 16 bytes and more of field header
    for w in (5, 6, 7, 8, 10):
        add(f"tag.w{w}.len.w10", vi(0x12, w) + vi(len(KEY), 10) + KEY + rest, marks=(w + 5,))
        add(f"tag.w{w}.num.w10", field(2, KEY) + field(4, 6) + field(5, 7) + vi(0x18, w) + vi((1 << 63) + 77),
            marks=(len(field(2, KEY)) + 4 + w + 5,))
        add(f"tag.w{w}.skip.w10", field(2, KEY) + vi(0x78, w) + vi((1 << 64) - 1) + vi(0x7a, w) + vi(2, 10) + b"ab" + rest)
    add("len.natural2", fields(key=b"K" * 200, value=b"V" * 300))

    # the numbers at the edges of the JS Number and of 64 bits
    big = [(1 << 53) - 1, 1 << 53, (1 << 53) + 1, (1 << 63) - 1, 1 << 63, (1 << 64) - 1]
    for i, v in enumerate(big):
        a, b, c = v, big[(i + 1) % 6], big[(i + 2) % 6]
        add(f"num.{v:#x}", fields(change=a, **{"from": b, "to": c}), marks=(len(field(2, KEY)) + 5,))

    # prefixes: ToInt32 wraps, 2^53 and beyond
    add("tag.wrap.key", vi((1 << 32) + 0x12) + vi(len(KEY)) + KEY + rest, marks=(2,))
    add("tag.wrap.key52", vi((1 << 52) + 0x12) + vi(len(KEY)) + KEY + rest, marks=(4,))
    add("tag.wrap.change", field(2, KEY) + vi((1 << 35) + 0x18) + vi(9) + field(4, 6) + field(5, 7))
    add("tag.negative.bytes", full + vi(0x80000012) + vi(3) + b"abc")
    add("tag.negative.varint", full + vi(0x80000010) + vi(1 << 60))
    add("tag.negative.wire7", full + vi((1 << 53) - 1))  # ToInt32 = -1: tag -1, wire type 7
    add("tag.2p53", full + vi(1 << 53) + b"\x00")
    add("tag.2p53.key", vi((1 << 53) + 0x12) + vi(len(KEY)) + KEY + rest, marks=(4,))
    add("tag.2p64m1", full + vi((1 << 64) - 1) + b"\x00")
    add("tag.zero", full + b"\x00\x05")  # tag 0, wire 0
    add("tag.seven", full + field(7, 1))

    # lengths at and above 2^53, and past the payload
    for t, nm in [(1, "subset"), (2, "key"), (6, "value"), (15, "unknown")]:
        pre = b"" if t == 2 else field(2, KEY)
        add(f"{nm}.len.2p53", pre + vi(t << 3 | 2) + vi(1 << 53) + b"xx" + rest)
        add(f"{nm}.len.2p53m1", pre + vi(t << 3 | 2) + vi((1 << 53) - 1) + b"xx" + rest)
        add(f"{nm}.len.2p64m1", pre + vi(t << 3 | 2) + vi((1 << 64) - 1) + b"xx" + rest)
        add(f"{nm}.len.past1", pre + rest + vi(t << 3 | 2) + vi(4) + b"abc")
        add(f"{nm}.len.exact", pre + rest + vi(t << 3 | 2) + vi(3) + b"abc")
        add(f"{nm}.len.u32wrap", pre + rest + vi(t << 3 | 2) + vi((1 << 32) + 3) + b"abc")

    # unknown tags by wire type
    add("unknown.all", full + b"\x48\x96\x01" + b"\x52\x03abc" + b"\x5d\x01\x02\x03\x04" + b"\x61" + bytes(8))
    add("unknown.first", b"\x48\x96\x01" + b"\x52\x03abc" + b"\x5d\x01\x02\x03\x04" + b"\x61" + bytes(8) + full)
    for w in (3, 4, 6, 7):
        add(f"unknown.wire{w}", full + bytes([9 << 3 | w]) + b"\x00")
        add(f"unknown.wire{w}.first", bytes([9 << 3 | w]) + b"\x00" + full)
    for cut in range(4):
        add(f"fixed32.cut{cut}", full + b"\x5d" + bytes(cut))
    for cut in range(8):
        add(f"fixed64.cut{cut}", full + b"\x61" + bytes(cut))
    add("fixed32.then_more", full + b"\x5d\x80\x80\x80\x80" + b"\x48\x01")
    add("fixed64.then_more", full + b"\x61" + b"\xff" * 8 + b"\x48\x01")
    add("unknown.bytes.past", full + b"\x52\x05abc")
    add("unknown.bytes.empty", full + b"\x52\x00")

    # every known tag under every wire type: the body is the tag's, not the wire type's
    for t, nm in NAMES.items():
        for w in range(8):
            body = CANON[nm] if nm != "subset" else SUBSET
            one = field(t, body, wire=w)
            others = b"".join(field(TAG[k], CANON[k]) for k in ["key", "change", "from", "to"] if k != nm)
            add(f"known.{nm}.wire{w}", others + one)

    # malformed varints in each position: ten bytes worth 2^64 or more, eleven bytes, cut
    over, eleven, eleven0 = b"\xff" * 9 + b"\x02", b"\xff" * 10 + b"\x01", b"\x80" * 10 + b"\x00"
    spots = {"tag": lambda v: field(2, KEY) + rest + v + b"\x01",
             "len": lambda v: b"\x12" + v + KEY + rest,
             "num": lambda v: field(2, KEY) + field(4, 6) + field(5, 7) + b"\x18" + v,
             "skip.varint": lambda v: full + b"\x48" + v,
             "skip.len": lambda v: full + b"\x52" + v + b"abc"}
    for spot, make in spots.items():
        add(f"{spot}.ge2p64", make(over))
        add(f"{spot}.ge2p64.7f", make(b"\xff" * 9 + b"\x7f"))
        add(f"{spot}.eleven", make(eleven))
        add(f"{spot}.eleven.zero", make(eleven0))
        if spot in ("num", "skip.varint"):
            add(f"{spot}.ten.max", make(b"\xff" * 9 + b"\x01"))
    head = field(2, KEY) + field(4, 6) + field(5, 7)
    for w in range(0, 11):  # the payload ends after w bytes of the varint (0: a lone tag byte)
        add(f"num.cut{w}", head + b"\x18" + b"\x80" * w)
        add(f"len.cut{w}", rest + b"\x12" + b"\xff" * w)
        add(f"skip.varint.cut{w}", full + b"\x48" + b"\x80" * w)
        add(f"skip.len.cut{w}", full + b"\x52" + b"\x81" * w)
        if w:
            add(f"tag.cut{w}", full + b"\x92" + b"\x80" * (w - 1))
    add("lone.tag.key", rest + b"\x12")
    add("lone.tag.only", b"\x18")
    return m


def reach_matrix(img):
    """Payloads whose later field headers lie more than `img` bytes (a kernel's LDS image) behind
    the payload's start, so that a decoder working from the image must go back to the stream for
    them; each also with a malformed field behind the long one."""
    m = []
    add = lambda name, payload: m.append(Entry(name, payload))
    rest = field(3, 5) + field(4, 6) + field(5, 7)
    tails = {"ok": b"", "wire3": b"\x4b\x00", "cut": b"\x48\x80\x80", "missing": None}
    long_ = lambda n, s: bytes((i * 7 + s) & 0xFF for i in range(n))
    for tn, tail in tails.items():
        if tail is None:  # the field behind the long one is absent: a required field missing
            add(f"value_first.{tn}", field(6, long_(img + 1, 1)) + field(5, 7) + field(4, 6) + field(2, KEY))
            add(f"long_key.{tn}", field(2, long_(img + 1, 2)) + field(3, 5) + field(4, 6))
            add(f"unknown9000.{tn}", field(2, KEY) + field(15, long_(9000, 3)) + field(4, 6) + field(5, 7))
            add(f"subset600.{tn}", field(1, long_(600, 4)) + field(2, KEY) + field(3, 5) + field(5, 7))
            continue
        add(f"value_first.{tn}", field(6, long_(img + 1, 1)) + field(5, 7) + field(4, 6) + field(3, 5) +
            field(2, KEY) + tail)
        add(f"long_key.{tn}", field(2, long_(img + 1, 2)) + rest + tail)
        add(f"unknown9000.{tn}", field(2, KEY) + field(15, long_(9000, 3)) + rest + tail)
        add(f"subset600.{tn}", field(1, long_(600, 4)) + field(2, KEY) + rest + tail)
    return m


def mutations(entries, seed, count):
    """`count` seeded mutations of the entries' payloads: byte flips, truncations, splices."""
    rng = random.Random(seed)
    small = [e.payload for e in entries if 0 < len(e.payload) <= 400]
    out = []
    while len(out) < count:
        p = bytearray(rng.choice(small))
        kind = rng.randrange(4)
        if kind == 0:
            for _ in range(rng.randint(1, 3)):
                p[rng.randrange(len(p))] ^= 1 << rng.randrange(8)
        elif kind == 1:
            p[rng.randrange(len(p))] = rng.choice([0, 0x7F, 0x80, 0xFF, rng.randrange(256)])
        elif kind == 2:
            p = p[:rng.randrange(len(p) + 1)]
        else:
            q = rng.choice(small)
            a, b = rng.randrange(len(p) + 1), rng.randrange(len(q) + 1)
            p = p[:a] + q[b:] if rng.random() < 0.5 else p[:a] + q[b:b + rng.randint(1, 12)] + p[a:]
        out.append(bytes(p))
    return out


if __name__ == "__main__":  # the coverage table: every branch label and the first entry that reaches it
    first = {}
    for e in change_matrix():
        for lab in decode(e.payload)["labels"]:
            first.setdefault(lab, e.name)
    for lab in sorted(LABELS):
        print(f"{lab:24s} {first.get(lab, '-- not reached --')}")
