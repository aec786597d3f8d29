"""CPU: the independent model of the Change payload decode (tests/_change_model.py, written from
the policy text) against the oracle (oracle_change_decode): on every entry of the matrix, on the
google.protobuf vectors of tests/golden/change_codec.json, on the long payloads of reach_matrix
and on seeded mutations. The matrix must walk every branch label of the model."""
import json
import os

import pytest

import _change_model as M
import _oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracle_row(p):
    c = O.change_decode(p)
    return {"key_off": c.key_off, "key_len": c.key_len, "subset_off": c.subset_off, "subset_len": c.subset_len,
            "value_off": c.value_off, "value_len": c.value_len, "change": c.change, "from": c.from_, "to": c.to,
            "flags": c.flags, "err": c.err}


def same(p, label):
    m = M.decode(p)
    o = oracle_row(p)
    for k, v in o.items():
        want = m[k] & 0xFFFFFFFF if k.endswith(("_off", "_len")) else m[k]  # (u32 columns)
        assert v == want, (label, k, v, want, p[:64].hex())
    return m


@pytest.fixture(scope="module")
def matrix():
    return M.change_matrix()


def test_names_are_unique(matrix):
    names = [e.name for e in matrix]
    assert len(set(names)) == len(names)


def test_model_equals_oracle_on_the_matrix(matrix):
    for e in matrix:
        same(e.payload, e.name)


def test_matrix_reaches_every_branch(matrix):
    hit = set()
    for e in matrix:
        hit |= M.decode(e.payload)["labels"]
    assert hit == M.LABELS, (sorted(M.LABELS - hit), sorted(hit - M.LABELS))


def test_matrix_outcomes(matrix):
    """What the policy says outright, read off the model: spot checks that do not pass through the
    oracle."""
    by = {e.name: M.decode(e.payload) for e in matrix}
    assert by["canonical"]["err"] == 0 and by["canonical"]["flags"] == M.F_VALUE
    assert by["empty"]["err"] == M.ERR_REQUIRED and by["empty"]["flags"] == M.F_BAD | M.F_MISSING
    assert by["tag.wrap.key"]["err"] == 0 and by["tag.wrap.key"]["key_len"] == 2
    assert by["tag.negative.bytes"]["err"] == 0
    assert by["tag.2p53.key"]["err"] == M.ERR_CHANGE
    assert by["num.0xffffffffffffffff"]["change"] == (1 << 64) - 1
    assert by["num.0x20000000000000"]["err"] == 0
    assert by["key.len.2p53"]["err"] == M.ERR_CHANGE
    assert by["dup.change"]["change"] == 300 and by["dup.change.first"]["change"] == 5
    for w in range(8):
        assert by[f"known.key.wire{w}"]["err"] == 0
    for w in (3, 4, 6, 7):
        assert by[f"unknown.wire{w}"]["err"] == M.ERR_CHANGE
    for k in M.REQUIRED:
        assert by[f"missing.{k}"]["err"] == M.ERR_REQUIRED


def test_model_equals_oracle_on_the_codec_vectors():
    vec = json.load(open(os.path.join(ROOT, "tests", "golden", "change_codec.json")))["vectors"]
    assert len(vec) >= 250
    for i, v in enumerate(vec):
        same(bytes.fromhex(v["payload"]), f"vector {i}")


def test_model_equals_oracle_on_long_payloads():
    for img in (4096 + 512, 8192 + 512):
        for e in M.reach_matrix(img):
            same(e.payload, e.name)


def test_model_equals_oracle_on_mutations(matrix):
    errs = set()
    for i, p in enumerate(M.mutations(matrix, seed=20, count=4000)):
        errs.add(same(p, f"mutation {i}")["err"])
    assert errs == {M.ERR_NONE, M.ERR_CHANGE, M.ERR_REQUIRED}
