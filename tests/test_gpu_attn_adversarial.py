"""Decode and extend attention over the quantised store on adversarial inputs (tests/attn_cases.py): attention sinks,
positional probes, q / k outlier channels, V scales over four decades and a late-moving score maximum, through every
decode route and both extend launch patterns (one split; splits + the log-sum-exp merge), each route asserted with the
kernel log. The check is the error budget of ``attn_cases.bound`` (the standard tolerance plus data-dependent terms for
what the kernels document: the exact dequantised values, P rounded to f16 / bf16 after the V-scale normalisation, the
two-plane INT8 query); tests/test_attn_discrimination.py shows that the same check rejects the mistakes that matter on
the same inputs."""
import numpy as np
import pytest

from tests import attn_cases as A
from tests.attn_cases import DECODE_ROUTES, EXTEND_ROUTES, KINDS
from tests.gpu_harness import K, run_case, tunable, within_standard  # noqa: F401

pytestmark = pytest.mark.gpu

# families: (name, make_case keyword arguments, also in bf16)
FAMILIES = [("sink", {}, True), ("probe", {}, True), ("outlier", {"factor": 16.0}, False),
            ("outlier", {"factor": 100.0}, False), ("vrange", {}, True), ("late", {}, False)]


def _assert_within(c, got, qplanes, what):
    ref = c.reference()
    ok, r = A.check(got, ref, A.bound(c, ref, qplanes=qplanes))
    assert ok, (what, c.info["family"], c.info["variant"], c.info["factor"], c.dtype, r)


def _cases(mode, shape, splits, seed, **kw):
    B, Hq, Hkv, T, S, D = shape
    for fam, extra, bf16 in FAMILIES:
        for dtype in ("f16", "bf16") if bf16 else ("f16",):
            yield A.make_case(fam, mode, B, Hq, Hkv, T, S, D, KINDS, dtype, seed=seed, splits=splits, **extra, **kw)


@pytest.mark.parametrize("route", list(DECODE_ROUTES))
def test_decode_routes_on_adversarial_inputs(K, tunable, route):
    (B, Hq, Hkv, T, D), knobs, kernel, splits = DECODE_ROUTES[route]
    for key, val in knobs.items():
        tunable(key, val)
    for c in _cases("decode", (B, Hq, Hkv, T, 1, D), splits, seed=len(route) + D):
        got, log, _ = run_case(K, c, "attn")
        assert log[0].startswith(kernel), (route, log)
        _assert_within(c, got, qplanes=kernel.startswith("decode_attn_partial_mfma_k<8") or kernel.startswith("decode_attn_lds"),
                       what=route)
        if c.info["family"] == "outlier" and c.info["factor"] == 16.0:  # 16 x outliers: the standard tolerance holds too
            within_standard(got, c.reference(), "f16", route)


def test_decode_step_dev_on_the_ring_on_adversarial_inputs(K, tunable):
    """kvq_decode_step_dev with the count on the device, on the ring kernel (attn_ring_dev = 1): count 1,000 under a
    bound of 3,100 at batch 8 (the ring by size; tiles per wave derived from the count)."""
    tunable("attn_ring_dev", 1)
    B, Hq, Hkv, T, D = 8, 32, 8, 1000, 128
    for fam, extra in (("sink", {}), ("probe", {}), ("vrange", {}), ("late", {})):
        c = A.make_case(fam, "decode", B, Hq, Hkv, T, 1, D, KINDS, "f16", seed=7, splits=(128, 256), probe_every=4, **extra)
        got, log, _ = run_case(K, c, "dev", bound=3100)
        assert log[0].startswith("decode_attn_lds_mfma_k<8, 4, 64, true, 2, 4, 128, true>") and log[1].endswith(", true>"), log
        _assert_within(c, got, qplanes=True, what="decode_step_dev ring")


@pytest.mark.parametrize("route", list(EXTEND_ROUTES))
def test_extend_on_adversarial_inputs(K, route):
    shape, want = EXTEND_ROUTES[route]
    B, Hq, Hkv, T, S, D = shape
    _, ns, per = A.extend_plan(B, Hq, Hkv, T, S)
    assert want is None or ns == want
    variants = [None, "chunk"]  # the sink once in the store, once in the chunk
    for c in _cases("extend", shape, (per * 64,) if per else (), seed=T + S):
        for var in variants if c.info["family"] == "sink" else [None]:
            if var:
                c = A.make_case("sink", "extend", B, Hq, Hkv, T, S, D, KINDS, c.dtype, seed=T + S + 1, splits=(per * 64,), variant=var)
            got, log, _ = run_case(K, c, "extend")
            assert log[0].startswith("extend_attn_k<") and (log[1:] == [] if ns == 1 else log[1].startswith("extend_attn_merge_k<")), log
            _assert_within(c, got, qplanes=False, what=route)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_extend_future_spike_leaves_earlier_rows_bit_identical(K, dtype):
    """A chunk token j with a huge score for every row of its kv head and a new V is in the future of rows s < j: their
    output is bit-identical to the same call without the spike; rows s >= j move to it."""
    B, Hq, Hkv, T, S, D = 1, 28, 4, 700, 9, 128
    c = A.make_case("probe", "extend", B, Hq, Hkv, T, S, D, KINDS, dtype, seed=5)
    base = run_case(K, c, "extend")[0]
    for j in (1, 4, S - 1):
        kn = A.widen(c.kn, dtype).astype(np.float32)
        qg = A.widen(c.q, dtype).reshape(B, Hkv, Hq // Hkv, S, D).sum(axis=(2, 3))  # [B,Hkv,D]: every row's query
        kn[:, :, j] += (40.0 / np.linalg.norm(qg, axis=-1, keepdims=True) * np.sqrt(D)) * qg
        vn = A.widen(c.vn, dtype).astype(np.float32)
        vn[:, :, j] = 8.0
        got = run_case(K, c, "extend", kn=A.narrow(kn, dtype), vn=A.narrow(vn, dtype))[0]
        assert np.array_equal(got[:, :, :j], base[:, :, :j]), j
        assert (np.abs(got[:, :, j:] - 8.0) < 0.1).all(), j
