"""CPU checks of tests/_claims.py, the model and case builders behind tests/test_gpu_claims_exact.py:
every stream is quiet and decodes without an error, every named case sits where it is named for,
the tile each case is named for is decidable (a condition on the inputs, nothing measured on a
GPU), the model agrees with the oracle's frame table, and the comparator names an altered entry.
An edit to a builder that loses a geometry, or to the model that makes it vacuous, fails here."""
import os
import re

import numpy as np
import pytest

import _claims as K
import _oracle as O

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dat-replication-protocol_amd", "csrc")
NAMES = sorted(K.FAMILIES)
# The hop walkers sync on shaped Changes only (walk_sync, drp_walk.hip): D's runs of blob frames and
# of id-0 headers hold none, so its tiles inside the runs are decidable for claims_fast / spec_claims
# alone. Every other family keeps the cap for both forms.
HOP_CAP = [n for n in NAMES if n != "D"]


def test_constants_match_the_kernels():
    spec = open(os.path.join(CSRC, "drp_spec.h")).read()
    dec = open(os.path.join(CSRC, "drp_decode_spec.hip")).read()
    dev = open(os.path.join(CSRC, "drp_device.h")).read()
    walk = open(os.path.join(CSRC, "drp_walk.hip")).read()
    assert int(re.search(r"#define DRP_SPEC_NT (\d+)", spec).group(1)) == K.NT
    assert int(re.search(r"SEGB = (\d+)", spec).group(1)) == K.SEGB
    assert int(re.search(r"HALO = (\d+)", spec).group(1)) == K.HALO
    assert int(re.search(r"#define DRP_FCAP (\d+)", dec).group(1)) == K.FCAP
    assert int(re.search(r"#define DRP_KSTRONG (\d+)", dec).group(1)) == K.KSTRONG
    assert int(re.search(r"SY_GENERAL = (\d+)", walk).group(1)) == K.SY_GENERAL
    for name, text in (("RDY", spec), ("C_ID", spec), ("M_ERR", spec), ("MARK_TERM", dev)):
        assert 1 << int(re.search(r"\b%s = 1ull << (\d+)" % name, text).group(1)) == getattr(K, name), name
    # the dump's layout (drp_launch_spec_head): 128 record bytes per tile and array
    assert re.search(r"hipMemcpy\(en\.data\(\), Q\.ent, ntl \* 128,", dec)


@pytest.mark.parametrize("name", NAMES)
def test_streams_are_quiet_and_decode_without_error(name):
    for ci, case in enumerate(K.family(name)):
        so, en = case["stream_off"], case["entry"]
        for s, m in enumerate(case["model"].streams):
            q, sh = K.quiet(m)
            assert q, (name, ci, s, [x for x in sh if x[2] != "dies"][:5])
            ref = O.decode_batch(case["wire"][so[s] + en[s]:so[s + 1]])
            assert ref["err_code"] == 0 and m.end != "error", (name, ci, s)
            # the model is the oracle's chain: counts, and every delivered frame's payload offset
            assert (m.nframes, m.nchanges) == (ref["nframes"], ref["changes"]), (name, ci, s)
            hdr = m.pos[m.deliv]
            vlen = np.array([K.parse_hdr(case["wire"], int(p), m.se)[2] for p in hdr], np.int64)
            np.testing.assert_array_equal(hdr + vlen + 1 - m.e0, ref["payload_off"][:m.nframes].astype(np.int64))
            assert {"end": 0}.get(m.end, ref["tail"]) == ref["tail"] and (m.end == "tail") == (ref["tail"] != 0)


@pytest.mark.parametrize("name", NAMES)
def test_model_is_self_consistent(name):
    """Per stream: the threads' frame and Change counts sum to the oracle's; every non-identity
    exit is the first chain position of the next tile that holds one, the tail, or the stream end."""
    for case in K.family(name):
        for m in case["model"].streams:
            n = c = 0
            firsts = {}
            for t in range(m.ntiles):
                ent, tn, tc = m.records(t)
                n += int(tn.sum())
                c += int(tc.sum())
                assert ((ent >= 0) | ((tn == 0) & (tc == 0))).all() and (tc <= tn).all()
                if (ent >= 0).any():
                    th = int(np.flatnonzero(ent >= 0)[0])
                    firsts[t] = m.base + t * K.TILE + th * K.SEGB + int(ent[th])
            assert (n, c) == (m.nframes, m.nchanges)
            assert sorted(firsts.values()) == sorted({int(p) for p in m.pos} & set(firsts.values()))
            for t in range(m.ntiles):
                cl = m.claim(t)
                assert (cl is None) == (t not in firsts)
                if cl is None:
                    continue
                later = [firsts[u] for u in sorted(firsts) if u > t]
                if cl[1]:
                    assert m.end == "tail" and cl[0] == int(m.pos[-1]) and not later
                elif later:
                    assert cl[0] == later[0]
                else:
                    assert cl[0] == m.se and m.end == "end"


@pytest.mark.parametrize("form", K.FORMS)
@pytest.mark.parametrize("name", NAMES)
def test_named_tiles_are_decidable(name, form):
    """The condition the GPU test stands on, per claims form a case is named for: every tile the
    case is named for is decidable, and at most 10 % of the tiles of the family's cases are not
    (tiles without a chain position are decidable: they must claim identity). Only D's runs of blob
    frames and of id-0 headers are named for one form alone: they hold no shaped Change, the hop
    walkers' only sync (walk_sync)."""
    tiles = und = 0
    for ci, case in enumerate(K.family(name)):
        if form not in case["forms"]:
            assert name == "D" and form == "hop" and ci < 2, (name, ci, form)
            continue
        M = case["model"]
        for g, s, t in M.tiles():
            tiles += 1
            und += not K.decidable(M.streams[s], t, form)[0]
        bad = [(s, t, K.decidable(M.streams[s], t, form)[2]) for s, t in case["named"]
               if not K.decidable(M.streams[s], t, form)[0]]
        assert case["named"] and not bad, (name, ci, form, bad)
    print(name, form, "tiles", tiles, "undecidable", und)
    assert tiles and und * 10 <= tiles, (name, form, und, tiles)


def test_family_a_is_what_it_is_named_for():
    """14 streams of at most 41 tiles, 523 tiles in all; a header of every varint width starts 1..k
    bytes before the tile end and before every halo block edge; the only live positions off the chain
    are inner bytes of multi-byte length varints, and each dies after exactly one frame."""
    where = []
    streams = K.straddle_streams(quiet=True, where=where, shaped=True)
    cases = K.family("A")
    assert [c["wire"] for c in cases] == streams and len(streams) == 14
    assert all(len(w) <= 41 * K.TILE for w in streams)
    assert sum(c["model"].ntiles for c in cases) == 523
    seen = set()
    for s, t, k, j, e in where:
        m = cases[s]["model"].streams[0]
        p = t * K.TILE + e - j
        assert p in m.chainset
        kind, fid, vlen, L, succ = K.parse_hdr(m.wire, p, m.se)
        assert (kind, fid, vlen) == (K.H_VALID, 1, k) and p < t * K.TILE + e < p + vlen + 1  # the edge cuts the header
        seen.add((k, j, e))
    assert seen == {(k, j, e) for k in (1, 2, 3) for j in range(1, k + 1) for e in range(0, K.HALO + 1, 16)}
    off_chain = empty = 0
    for c in cases:
        m = c["model"].streams[0]
        for q, frames, how in K.quiet(m)[1]:
            off_chain += 1
            assert (frames, how) == (1, "dies")
            assert any(q - d in m.chainset and all(m.wire[q - d + i] >= 0x80 for i in range(d)) for d in (1, 2)), q
        empty += sum(m.claim(t) is None for t in range(m.ntiles))
        assert all(K.decidable(m, t, form)[0] for t in range(m.ntiles) for form in K.FORMS)
    print("family A: off-chain live positions", off_chain, "tiles without a chain position", empty)
    assert off_chain == 476 and empty == 102


def test_family_b_frames_start_in_the_images_last_bytes():
    m = K.family("B")[0]["model"].streams[0]
    for d in range(1, 20):
        assert (d + 1) * K.TILE + K.HALO - d in m.chainset  # tile d's image ends at (d + 1) * TILE + HALO


def test_family_c_covers_every_offset_and_thread():
    m = K.family("C")[0]["model"].streams[0]
    offs, threads, edge = set(), set(), set()
    for t in range(1, m.ntiles - 1):
        ent, n, c = m.records(t)
        for th in np.flatnonzero(ent >= 0):
            offs.add(int(ent[th]))
            threads.add(int(th))
            p = m.base + t * K.TILE + th * K.SEGB + int(ent[th])
            vlen = K.parse_hdr(m.wire, p, m.se)[2]
            if int(ent[th]) + vlen + 1 > K.SEGB:  # the header (varint + id) crosses the thread's edge
                edge.add((int(ent[th]), vlen))
    assert offs == set(range(64)) and threads == set(range(K.NT))
    assert {(63, 1), (63, 2), (62, 2)} <= edge, edge
    assert all(np.gcd(flen, 64) == 1 for flen, _ in K.C_RUNS)


def test_family_d_dense_and_empty_threads():
    blobs, zeros, cap0, cap1 = (c["model"].streams[0] for c in K.family("D"))
    for t in (2, 3):  # tile 2 lies inside the runs, tile 3 holds their end: both past FCAP (spec_claims' general form)
        ent, n, c = blobs.records(t)
        assert {21, 22} <= set(n.tolist()) and n.sum() > K.NT and not c[:60].any()
        assert K.live_count(blobs.wire, t * K.TILE, t * K.TILE + K.IMG - 16) > K.FCAP
        ent, n, c = zeros.records(t)
        assert (ent[:60] >= 0).all() and not n[:60].any()  # carriers that deliver nothing
        assert K.live_count(zeros.wire, t * K.TILE, t * K.TILE + K.IMG - 16) > K.FCAP
    assert set(blobs.records(2)[1].tolist()) == {21, 22} and (zeros.records(2)[0] >= 0).all()
    assert K.live_count(cap0.wire, K.TILE, K.TILE + K.IMG - 16) == K.FCAP
    assert K.live_count(cap1.wire, K.TILE, K.TILE + K.IMG - 16) == K.FCAP + 1
    for m in (cap0, cap1):  # the seeds parse as one frame and land on an error header
        sh = [x for x in K.quiet(m)[1] if K.TILE <= x[0] < 2 * K.TILE]
        assert len(sh) >= K.FCAP - 40 and all((f, how) == (1, "dies") for _, f, how in sh)


def test_family_e_long_frames():
    m = K.family("E")[0]["model"].streams[0]
    assert [m.claim(t) is None for t in (2, 5, 6, 7)] == [True] * 4  # inside the long Change and the blob
    starts = {int(p) for p in m.pos}
    assert 13 * K.TILE + 100 in starts and K.parse_hdr(m.wire, 13 * K.TILE + 100, m.se)[3] > 4096  # in tile 12's halo
    p = 15 * K.TILE - 700
    assert p in starts and K.parse_hdr(m.wire, p, m.se)[4] > 14 * K.TILE + K.IMG  # the blob leaves tile 14's image
    long_in_tile = [int(q) for q in m.pos if 9 * K.TILE <= q < 12 * K.TILE and K.parse_hdr(m.wire, int(q), m.se)[3] > 4096]
    assert len(long_in_tile) >= 5 and all(K.shaped(m.wire, q, m.se) for q in long_in_tile)


def test_family_f_stream_edges():
    case = K.family("F")[0]
    M, so = case["model"], case["stream_off"]
    s0, s1, s2 = M.streams[1], M.streams[3], M.streams[5]
    assert all(so[s] % K.TILE for s in (1, 3, 5)) and case["entry"][1] == 777 and s0.e0 == so[1] + 777
    assert [m.err for m in (s0, s1, s2)] == [K.H_TAIL_HDR, K.H_TAIL_CHANGE, K.H_TAIL_BLOB]
    for m in (s0, s1, s2):
        last = m.ntiles - 1
        cl = m.claim(last)
        assert cl == (int(m.pos[-1]), True)  # the last tile's claim ends the chain at the tail
        a, i, j = m.tile_range(last)
        assert j - i > K.KSTRONG + 1  # more than KSTRONG whole frames before the tail in its tile
    assert s2.deliv[-1] and not s1.deliv[-1] and not s0.deliv[-1]  # a cut blob is delivered


def test_family_g_dead_shadows():
    m = K.family("G")[0]["model"].streams[0]
    sh = {q: (f, how) for q, f, how in K.quiet(m)[1]}
    same_segment = 0
    for p in m.pos[(m.pos >= K.TILE) & (m.pos < 4 * K.TILE)].tolist():
        q = p - 10
        if q in sh:
            assert sh[q] == (1, "dies") and m.wire[q:q + 2] == b"\x05\x01"
            kind = K.parse_hdr(m.wire, q + 6, m.se)[0]
            assert kind == K.H_ERR_TYPE
            same_segment += q // K.SEGB == p // K.SEGB
    assert same_segment > 200  # the seeded candidate precedes the real header in the thread's own bytes


# ---- the comparator is not vacuous -------------------------------------------------------------
def _dump_of(case, tmp_path, alter=None):
    path = str(tmp_path / "model.bin")
    K.write_dump(path, case["model"])
    if alter:
        raw = bytearray(open(path, "rb").read())
        alter(raw, case["model"].ntiles)
        open(path, "wb").write(bytes(raw))
    blocks = K.read_dump(path)
    assert len(blocks) == 1
    return K.compare(blocks[0], case["model"], "fast")


def test_comparator_accepts_the_model_and_names_an_altered_entry(tmp_path):
    case = K.family("C")[0]
    m = case["model"].streams[0]
    ntl = case["model"].ntiles
    assert _dump_of(case, tmp_path) == []
    tile = 2
    ent, n, c = m.records(tile)
    th = int(np.flatnonzero(ent >= 0)[5])
    claims, ents = 8, 8 + 8 * ntl

    def ent_byte(raw, ntl):
        raw[ents + tile * K.NT + th] ^= 1

    def ent_n(raw, ntl):
        raw[ents + ntl * K.NT + tile * K.NT + th] += 1

    def claim_shift(raw, ntl):
        raw[claims + 8 * tile] ^= 1  # (the position's low bit: one byte off)

    assert _dump_of(case, tmp_path, ent_byte) == [(tile, th, "ent", int(ent[th]) ^ 1, int(ent[th]))]
    assert _dump_of(case, tmp_path, ent_n) == [(tile, th, "ent_n", int(n[th]) + 1, int(n[th]))]
    want = m.claim(tile)[0]
    assert _dump_of(case, tmp_path, claim_shift) == [(tile, -1, "claim", want ^ 1, want)]
    # a restart bit on a later carrier, and a record where the model has none
    later = int(np.flatnonzero(ent >= 0)[9])

    def restart(raw, ntl):
        raw[ents + tile * K.NT + later] |= 0x40

    assert _dump_of(case, tmp_path, restart) == [(tile, later, "restart", int(ent[later]) | 0x40, int(ent[later]))]


def test_comparator_names_a_swapped_identity_claim(tmp_path):
    case = K.family("E")[0]
    m = case["model"].streams[0]
    tile = 6  # inside the three-tile blob: identity
    assert m.claim(tile) is None

    def swap(raw, ntl):
        raw[8 + 8 * tile:16 + 8 * tile] = (K.RDY | (7 * K.TILE + 3)).to_bytes(8, "little")

    assert _dump_of(case, tmp_path, swap) == [(tile, -1, "claim", hex(7 * K.TILE + 3), "identity")]
    other = 9  # a position claim swapped for identity

    def unswap(raw, ntl):
        raw[8 + 8 * other:16 + 8 * other] = (K.RDY | K.C_ID).to_bytes(8, "little")

    assert _dump_of(case, tmp_path, unswap) == [(other, -1, "claim", "identity", m.claim(other)[0])]


def test_dump_reader_takes_several_blocks(tmp_path):
    case = K.family("G")[0]
    path = str(tmp_path / "two.bin")
    K.write_dump(path, case["model"])
    K.write_dump(path, case["model"], mode="ab")
    blocks = K.read_dump(path)
    assert len(blocks) == 2 and all(K.compare(b, case["model"], "fast") == [] for b in blocks)
