"""GPU parity of the record emission across repair passes (verify_lite's tile_recok -> emit_recs,
drp_decode_spec.hip) against the oracle. emit_recs takes a tile's rows from claims_fast's record
slots, from slot sb on: sb is the sum of the per-thread frame counts (ent_n) of the threads before
the entry thread, and the slots were laid out from the counts claims_fast saw. Every path that
rewrites ent / ent_n after claims must therefore leave the tile without records (tile_rec REC_NONE;
DESIGN.md "Record slots and repair passes").

The streams are tests/_streams.merge_site's (geometry pinned by tests/test_merge_site.py): a host
frame whose payload holds a second framing that ends exactly where the host does. The tiles inside
the payload claim the second framing's exits and miss; tile t's entry, found by look-back, is the
predicted entry of its thread k, with the second framing's frames recorded by the threads before
it (sb > 0): verify_counts' fast path takes tile t in the dirty-list pass. A never-merging segment
further down (shadow_stream) then keeps missing one tile per pass until the host runs the
segmented repair and a full verify pass, in which verify_lite sees tile t again."""
import functools
import random
import re
import time

import numpy as np
import pytest

import _oracle as O
import _streams as S
from _tail import cut_entries, device_decode_check, stream_refs, tail_ctx

pytestmark = pytest.mark.gpu

KS = [1, 2, 63, 64, 65, 127]
# 100-byte chain frames: four in a row inside the image make the chain strong (KSTRONG), one header
# per 64-byte segment at the most, 82 to 95 frames in tile t (tests/test_merge_site.py)
SLEN = 100
PRE, POST = 150, 200
# 95 C2 frames end 22 bytes before a tile's end: the host's header is that tile's last frame and the
# chain starts in the next tile, so the header's tile holds the real framing only
PRE_EDGE = 95
# periods of the never-merging segment: each verify pass repairs one of its tiles, so with 12 the
# head's pass and the three dirty-list passes behind it (kChain) all miss, the host then runs the
# segmented repair (kSegRepairAfter = 3) and one full pass: 4 repair passes, 1 segmented repair
SHADOW_N = 12


def whole(k):
    return 2 if k in (2, 65) else 1


@pytest.fixture(scope="module")
def ctxs():
    """Contexts by (records, environment), opened once (tests/_tail.tail_ctx)."""
    cache = {}

    def get(rec=1, **env):
        key = (rec, tuple(sorted(env.items())))
        if key not in cache:
            cache[key] = tail_ctx(rec, **env)
        return cache[key]
    yield get
    for c in cache.values():
        c.close()


@functools.lru_cache(maxsize=None)
def site(host, kind, k, slen=SLEN, chain=True, pre=PRE):
    return S.merge_site(pre, k, slen, kind, host, whole(k), POST, seed=31 + k, chain=chain)


def _kw(k, kind="narrow", host="blob", post=POST):
    return dict(pre_frames=PRE, k=k, slen=SLEN, kind=kind, host=host, whole_tiles=whole(k), post_frames=post)


@functools.lru_cache(maxsize=None)
def cascade(name):
    """The cascade wires: sites, C2 frames, the never-merging segment, C2 frames."""
    if name == "one":
        return S.site_cascade([_kw(64)], shadow_n=SHADOW_N)
    if name == "two":
        return S.site_cascade([_kw(2, "wide", "change"), _kw(127, "blob")], shadow_n=SHADOW_N)
    if name == "after":  # the second site lies inside the segmented repair's range
        return S.site_cascade([_kw(63, "wide")], shadow_n=SHADOW_N, after=[_kw(65, "narrow", "change")])
    if name == "last":  # tile t is the stream's last tile
        w, m = S.site_cascade([_kw(64, "blob")], shadow_n=SHADOW_N, after=[_kw(64, post=20)], tail_frames=0)
        assert (len(w) - 1) // S.TILE == m[-1]["t"]
        return w, m
    raise KeyError(name)


CASCADE_NAMES = ["one", "two", "after", "last"]


@functools.lru_cache(maxsize=None)
def oracle(fn, *args):
    return O.decode_batch(fn(*args)[0])


def check(ctx, fn, *args, label=None):
    """One decode against the oracle, every row and column; returns the decode's timing."""
    from _gpu import assert_same
    t0 = time.perf_counter()
    g = ctx.decode_batch(fn(*args)[0])
    dt = time.perf_counter() - t0
    t = ctx.timing()
    print(f"{label or args}: {len(fn(*args)[0])} B, {dt * 1e3:.1f} ms, repair passes {t.spec_repairs}, "
          f"segmented {t.seg_repairs}, exact re-runs {t.strict_reruns}")
    r = oracle(fn, *args)
    n = min(len(g["payload_off"]), len(r["payload_off"]))
    bad = np.flatnonzero((g["payload_off"][:n] != r["payload_off"][:n]) | (g["payload_len"][:n] != r["payload_len"][:n]))
    if len(bad):
        i = int(bad[0])
        print(f"{label or args}: first differing row {i}: payload_off {int(g['payload_off'][i])} len "
              f"{int(g['payload_len'][i])}, the oracle's {int(r['payload_off'][i])} len {int(r['payload_len'][i])}")
    assert_same(g, r, str(label or args))
    assert t.strict_reruns == 0, "fell back to the exact kernel"
    return t


# ---- the entry slot with frames before it (sb > 0), no later pass ----------------------------------

@pytest.mark.parametrize("rec", [1, 0])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("kind", S.SITE_KINDS)
@pytest.mark.parametrize("host", S.SITE_HOSTS)
def test_site_alone(ctxs, host, kind, k, rec):
    t = check(ctxs(rec=rec), site, host, kind, k)
    assert t.spec_repairs >= 1  # the prediction followed the second framing


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("host", S.SITE_HOSTS)
def test_site_alone_header_at_tile_end(ctxs, host, k):
    """The host's header as the last frame of its tile: that tile predicts the real framing."""
    t = check(ctxs(), site, host, "narrow", k, SLEN, True, PRE_EDGE)
    # (k = 1, one payload tile: the chain's last frame of tile t - 1 ends where the host does, so that
    # tile's exit is the real entry whichever framing it followed, and nothing has to miss)
    assert t.spec_repairs >= 1 or (k == 1 and whole(k) == 1)


@pytest.mark.parametrize("kind", ["blob", "narrow"])
def test_site_without_records(ctxs, kind):
    """The no-records control: 40-byte chain frames, more than 128 frames in tile t."""
    t = check(ctxs(), site, "blob", kind, 127, 40)
    assert t.spec_repairs >= 1


@pytest.mark.parametrize("host", S.SITE_HOSTS)
def test_site_filler_control(ctxs, host):
    """Random filler in place of the chain: no second framing, no repair."""
    t = check(ctxs(), site, host, "narrow", 64, SLEN, False)
    assert t.spec_repairs == 0


# ---- the fast path, then a full pass ------------------------------------------------------------------

@pytest.mark.parametrize("name", CASCADE_NAMES)
def test_fast_path_then_full_pass(ctxs, name):
    t = check(ctxs(), cascade, name)
    assert t.spec_repairs >= 4 and t.seg_repairs >= 1, (t.spec_repairs, t.seg_repairs)


@pytest.mark.parametrize("name", CASCADE_NAMES)
def test_fast_path_then_full_pass_without_records(ctxs, name):
    check(ctxs(rec=0), cascade, name)


# ---- other ways to a full pass ------------------------------------------------------------------------

ENVS = [{"DRP_DIRTY_CAP": "0"}, {"DRP_DIRTY_CAP": "1"}, {"DRP_DIRTY_CAP": "2"}, {"DRP_CASCADE_MIN": "1"}]


@pytest.mark.parametrize("env", ENVS, ids=lambda e: "-".join(f"{k[4:].lower()}{v}" for k, v in e.items()))
@pytest.mark.parametrize("name", CASCADE_NAMES)
def test_full_pass_by_knob(ctxs, name, env):
    """A dirty list past its capacity (every repair pass a full one), and the head's cascade
    shortcut (the segmented repair from the first listed tile, which is the site's)."""
    check(ctxs(**env), cascade, name, label=f"{name} {env}")


@functools.lru_cache(maxsize=None)
def blob_run(k):
    """A site, then tests/test_gpu_cascade.py's blob run behind a second miss: 4 KB Changes around a
    600 KB blob of two-byte frames, whose repair lists 64 identity tiles and sets the dirty list's
    overflow word, so a later pass is a full one (measured: 4 repair passes, 1 segmented repair; the
    site's tile was taken by the dirty-list pass before, so the full pass sees it again)."""
    w, m = site("blob", "narrow", k)
    rng = random.Random(7)
    parts = [S.frame(S.change_payload(b"k%06d" % i, i + 1, i, i + 1, rng.randbytes(4096))) for i in range(300)]
    parts.insert(150, S.frame(b"\x01\x02" * 300_000, 2))
    return w + b"".join(parts), m


@pytest.mark.parametrize("k", [2, 64, 127])
def test_full_pass_by_identity_run(ctxs, k):
    t = check(ctxs(), blob_run, k)
    assert t.spec_repairs >= 2  # (the site's dirty-list pass, and a pass after the blob's miss)


# ---- reach, from the library's own report -------------------------------------------------------------

def stats_decode(wire, ref, label):
    """One decode on a context opened with DRP_STATS=1 (it prints the first five misses to stderr)."""
    from _gpu import assert_same
    c = tail_ctx(1, DRP_STATS="1")
    try:
        g = c.decode_batch(wire)
    finally:
        c.close()
    assert_same(g, ref, label)


@pytest.mark.parametrize("k", [64, 65])
@pytest.mark.parametrize("pre", [PRE_EDGE, PRE])
def test_first_miss_is_the_payload_tile(capfd, pre, k):
    """DRP_STATS=1 prints the first misses. With the host's header at its tile's end (PRE_EDGE) the
    first miss is tile t - whole_tiles, the first tile inside the payload: it claims the second
    framing's exit while the real entry passes through it. Every tile up to t - 1 does the same, one
    per pass, and nothing else misses. With chain frames behind the header in the header's own tile
    (PRE), that tile prefers the chain as well (the denser framing) and misses first."""
    args = ("blob", "narrow", k, SLEN, True, pre)
    wire, m = site(*args)
    capfd.readouterr()
    stats_decode(wire, oracle(site, *args), f"stats {pre} {k}")
    err = capfd.readouterr().err
    line = [ln for ln in err.split("\n") if ln.startswith("[drp-spec] misses=")]
    assert len(line) == 1, err
    print(line[0][:line[0].index(" walk:")])
    n = int(re.match(r"\[drp-spec\] misses=(\d+)", line[0]).group(1))
    tiles = [int(x) for x in re.findall(r"\| t=(\d+) ", line[0])]
    t, w = m["t"], m["whole_tiles"]
    first = t - w if pre == PRE_EDGE else t - w - 1
    assert tiles[0] == first, (tiles, m)
    assert n == len(tiles) and tiles == list(range(first, t)), (n, tiles, m)


# ---- other callers of the same tail -------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def cut_case(where):
    """The cascade wire as three streams, the site in the middle one: the first cut inside the
    host frame (the middle stream enters at the frame after the host, the chain before its entry),
    or before the site's last C2 frames; the second cut in the C2 frames after the segment."""
    wire, (m,) = cascade("one")
    c1 = m["host_start"] + 3000 if where == "host" else 86 * (PRE - 20) + 11
    c2 = m["shadow"][1] + 86 * 100 + 40
    cuts = [0, c1, c2, len(wire)]
    entry, nrows = cut_entries(wire, cuts)
    if where == "host":
        assert cuts[1] + entry[1] == m["host_end"]
    return wire, cuts, entry, stream_refs(wire, cuts, entry), nrows


@pytest.mark.parametrize("where", ["host", "before"])
def test_three_streams(ctxs, where):
    device_decode_check(ctxs(), *cut_case(where))


@pytest.mark.parametrize("name", CASCADE_NAMES)
def test_staged_pieces(ctxs, name):
    from _gpu import assert_same
    c = ctxs()
    g = c.decode_staged(cascade(name)[0], pieces=3)
    assert c.timing().strict_reruns == 0
    assert_same(g, oracle(cascade, name), f"staged {name}")


def test_exact_kernel_cross_check():
    """The exact decode (no prediction, no records) of the cascade wire: the oracle's rows too."""
    from _gpu import assert_same
    c = tail_ctx(1)
    try:
        c.set_exact(True)
        assert_same(c.decode_batch(cascade("two")[0]), oracle(cascade, "two"), "exact")
    finally:
        c.close()


# ---- same context, next batch -------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def clean_wire():
    return S.c2_stream(3001, seed=5).tobytes(), None


@pytest.mark.parametrize("rec", [1, 0])
def test_next_batch_on_one_context(ctxs, rec):
    """The cascade wire, a clean wire of another tile count, the cascade wire again: tile_rec and
    tile_recok of the batch before are left in the scratch."""
    assert len(cascade("two")[0]) // S.TILE != len(clean_wire()[0]) // S.TILE
    c = ctxs(rec=rec)
    check(c, cascade, "two")
    t = check(c, clean_wire)
    assert t.spec_repairs == 0
    check(c, cascade, "two")
    check(c, cascade, "after")
