"""The claims kernels' own output against the exact-chain model (tests/_claims.py).

claims_fast, spec_claims and the hop walkers write every tile's claim and the per-thread entry
records; verification then proves them and the repair passes correct what was wrong, so a claims
kernel that predicts wrongly still delivers the oracle's rows, only slower. Here the library dumps
what those kernels wrote, before verification touches it (DRP_DUMP_CLAIMS, drp_launch_spec_head),
and every tile whose prediction follows from the bytes (decidable(), each rule cited there) must
equal the model: the claim's position and MARK_TERM, every thread's entry offset, frame and Change
counts, and no restart bit after the tile's first carrier. Rows are the oracle's and no repair pass
runs. Each claims form (DRP_CLAIMS=fast, or hop with DRP_WALK_MIN=0) runs with per-frame records on
and off (DRP_CREC) and with claims_fast's structural check of long Changes on and off
(DRP_CHANGE_CHECKS): all four claims_fast<CF, REC> instantiations. tests/test_claims_cases.py proves
on the CPU that the inputs are what they are named for."""
import os

import pytest

import _claims as K
import _oracle as O
import _tail as T

pytestmark = pytest.mark.gpu

ENV = ("DRP_CLAIMS", "DRP_WALK_MIN", "DRP_CREC", "DRP_CHANGE_CHECKS")
PARAMS = [(form, crec, cc) for form in ("fast", "hop") for crec in (1, 0) for cc in (1, 0)]


def open_ctx(form, crec, cc):
    from _gpu import drp_amd
    env = {"DRP_CLAIMS": form, "DRP_WALK_MIN": "0", "DRP_CREC": str(crec), "DRP_CHANGE_CHECKS": str(cc)}
    keep = {k: os.environ.get(k) for k in ENV}
    os.environ.update(env)
    try:
        c = drp_amd.Ctx(0)
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    c.set_blob_skip(0)  # (every batch staged whole: one head launch sees all of it)
    return c


@pytest.fixture(scope="module", params=PARAMS, ids=["%s-crec%d-cc%d" % p for p in PARAMS])
def ctx(request):
    c = open_ctx(*request.param)
    c.form = request.param[0]
    yield c
    c.close()


def dumped(path, fn):
    """fn() with DRP_DUMP_CLAIMS set to the fresh file `path`; the dump's blocks."""
    assert not os.path.exists(path)
    os.environ["DRP_DUMP_CLAIMS"] = path
    try:
        out = fn()
    finally:
        os.environ.pop("DRP_DUMP_CLAIMS", None)
    return out, K.read_dump(path)


def check_timing(ctx, label):
    t = ctx.timing()
    assert (t.spec_repairs, t.strict_reruns, t.seg_repairs) == (0, 0, 0), (label, t.spec_repairs, t.strict_reruns,
                                                                          t.seg_repairs)


def check_dump(blocks, case, form, label):
    assert len(blocks) == 1, (label, "head launches", len(blocks))
    bad = K.compare(blocks[0], case["model"], form)
    assert not bad, (label, len(bad), bad[:12])


def decode_host(ctx, case, path, label):
    from _gpu import assert_same
    wire = case["wire"]
    got, blocks = dumped(path, lambda: ctx.decode_batch(wire))
    assert_same(got, O.decode_batch(wire, chunk=65536), label)
    check_dump(blocks, case, ctx.form, label)
    check_timing(ctx, label)


def decode_on_device(ctx, case, path, label):
    """Several streams in one drp_decode_device call: tests/_tail.py's device decode, which checks
    every stream's result and every row against the per-stream oracle decodes."""
    wire, so, entry = case["wire"], case["stream_off"], case["entry"]
    refs = T.stream_refs(wire, so, entry)
    nrows = sum(r["nframes"] for r in refs)
    _, blocks = dumped(path, lambda: T.device_decode_check(ctx, wire, so, entry, refs, nrows))
    check_dump(blocks, case, ctx.form, label)
    check_timing(ctx, label)


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E", "G"])
def test_family(ctx, name, tmp_path):
    """A: headers across the tile end and every halo block edge; B: frames starting in the image's
    last 19 bytes; C: carriers at every offset and in every thread; D: dense and empty threads, the
    list's capacity; E: long frames; G: dead shadows before a real header."""
    for i, case in enumerate(K.family(name)):
        # (D's three- and two-byte frames are more rows than a host batch's capacity guess, stage_cap:
        # drp_decode_batch would decode them twice, two head launches; the device call takes the
        # capacity from the caller)
        run = decode_on_device if name == "D" else decode_host
        run(ctx, case, str(tmp_path / ("claims%d.bin" % i)), "%s%d" % (name, i))


def test_family_f_stream_edges(ctx, tmp_path):
    """Three streams at unaligned offsets in one call: a non-zero entry, and a header, a Change and
    a blob tail."""
    for i, case in enumerate(K.family("F")):
        decode_on_device(ctx, case, str(tmp_path / ("claims%d.bin" % i)), "F%d" % i)
