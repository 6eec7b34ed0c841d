"""The cases of tests/store_evict_cases.py must reject the mistakes a chunk summary inside the quantised store can make:
every mistake changes at least one output code byte or stored-scale word in EVERY case of the family designated for it.
CPU only: model and mistakes are numpy (the model is the composition of the oracle's own functions)."""
import numpy as np
import pytest

from tests import store_evict_cases as C

BUILT = {}


def _built(i):
    if i not in BUILT:
        fam, kw = C.CASES[i]
        case = C.build(fam, kw)
        BUILT[i] = (case, C.model(case))
    return BUILT[i]


IDS = [C.case_id(f, kw) for f, kw in C.CASES]


@pytest.mark.parametrize("i", range(len(C.CASES)), ids=IDS)
def test_mutant_defaults_are_the_model(i):
    case, want = _built(i)
    assert not C.differs(C.mutant(case), want)


@pytest.mark.parametrize("i", range(len(C.CASES)), ids=IDS)
def test_model_shapes_and_tail(i):
    case, (q, s) = _built(i)
    T = case["q"].shape[3]
    keep = min(case["keep"], T)
    old = T - keep
    n = -(-old // case["chunk"])
    assert q.shape[3] == n + keep == s.shape[1] and q.dtype == case["q"].dtype and s.dtype == np.float32
    assert np.array_equal(q[:, :, :, n:], case["q"][:, :, :, old:])
    assert np.array_equal(s[:, n:].view(np.uint32), case["s"][:, old:].view(np.uint32))


@pytest.mark.parametrize("mistake", list(C.MISTAKES))
def test_every_case_of_the_designated_family_rejects_the_mistake(mistake):
    kw, fam = C.MISTAKES[mistake]
    ran = 0
    for i, (f, ckw) in enumerate(C.CASES):
        if f != fam or (mistake == "nibbles_swapped" and ckw["kind"] != "int4"):
            continue
        case, want = _built(i)
        assert C.differs(C.mutant(case, **kw), want), (mistake, IDS[i])
        ran += 1
    assert ran >= 2


def test_families_are_what_they_say():
    for i, (fam, kw) in enumerate(C.CASES):
        case, (q, s) = _built(i)
        kind, D, chunk = case["kind"], case["D"], case["chunk"]
        codes = C.O.unpack_int4(case["q"], D) if kind == "int4" else case["q"]
        if fam == "zero":  # the first chunk is all zero: its scale is the stored eps
            assert not codes[:, :, :, :chunk].any()
            assert np.array_equal(s[:, 0], C.rt(np.full(s.shape[0], C.EPS, np.float32), case["dtype"]))
            assert (q[:, :, :, 0] == (0 if kind == "int8" else 0x88)).all()
        if fam == "extremes":
            assert (codes.max(axis=4) == C.QMAX[kind]).all() and (codes.min(axis=4) == C.QMIN[kind]).all()
        if fam == "scale_span":
            old = codes.shape[3] - case["keep"]
            sp = case["s"][:, :chunk]
            assert (sp.max(axis=1) / sp.min(axis=1) > 100).all()
            assert np.abs(codes[:, :, :, old:]).max() < C.QMAX[kind]
        if fam == "rounding":  # float(code) * scale is no dtype value (INT4: unless the code is 0 or a power of two)
            x = codes.astype(np.float32) * case["s"][:, None, None, :, None]
            assert (C.rt(x, case["dtype"]) != x).mean() > (0.5 if kind == "int8" else 0.25)
        if fam == "ragged":
            assert (codes.shape[3] - case["keep"]) % chunk in (1, chunk - 1) and chunk & (chunk - 1)
