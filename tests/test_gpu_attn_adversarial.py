"""Decode and extend attention over the quantised store on adversarial inputs (tests/attn_cases.py): attention sinks,
positional probes, q / k outlier channels, V scales over four decades and a late-moving score maximum, through every
decode route and both extend launch patterns (one split; splits + the log-sum-exp merge), each route asserted with the
kernel log. The check is the error budget of ``attn_cases.bound`` (the standard tolerance plus data-dependent terms for
what the kernels document: the exact dequantised values, P rounded to f16 / bf16 after the V-scale normalisation, the
two-plane INT8 query); tests/test_attn_discrimination.py shows that the same check rejects the mistakes that matter on
the same inputs."""
import numpy as np
import pytest
import torch

from tests import attn_cases as A
from tests.util import TD, to_numpy, to_torch

pytestmark = pytest.mark.gpu

KINDS = ("int8", "int4")

# decode routes: name -> (B, Hq, Hkv, T, D, tunables, kernel-log prefix, tokens per split)
DECODE_ROUTES = {
    "one-tile MFMA": ((2, 32, 8, 600, 128), {"attn_stream_tpw": -1}, "decode_attn_partial_mfma_k<8, 4, 128, 128, false>", (128,)),
    "ring hd128 TG4": ((2, 32, 8, 600, 128), {"attn_stream_tpw": 2}, "decode_attn_lds_mfma_k<8, 4, 64, true, 2, 4, 128, false>", (128,)),
    "ring hd128 TG1": ((2, 16, 2, 600, 128), {"attn_stream_tpw": 3}, "decode_attn_lds_mfma_k<8, 4, 64, true, 2, 1, 128, false>", (192,)),
    "ring hd64": ((2, 32, 8, 600, 64), {"attn_stream_tpw": 2}, "decode_attn_lds_mfma_k<8, 4, 64, true, 2, 4, 64, false>", (128,)),
    "VALU hd32": ((2, 16, 4, 600, 32), {}, "decode_attn_partial_k<8, 4, 4>", (512,)),
    "VALU hd256": ((2, 16, 4, 300, 256), {}, "decode_attn_partial_k<8, 4, 4>", (64,)),
}
# families: (name, make_case keyword arguments, also in bf16)
FAMILIES = [("sink", {}, True), ("probe", {}, True), ("outlier", {"factor": 16.0}, False),
            ("outlier", {"factor": 100.0}, False), ("vrange", {}, True), ("late", {}, False)]


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available()
    from efficient_llm_inference_amd import _lib, kernels
    _lib.load()
    return kernels


@pytest.fixture
def tunable():
    from efficient_llm_inference_amd import _lib
    touched = {}

    def set_(key, value):
        touched.setdefault(key, _lib.get_tunable(key))
        _lib.set_tunable(key, value)
    yield set_
    for key, old in touched.items():
        _lib.set_tunable(key, old)


def _stores(K, c, pad=3):
    """device stores with guard codes and NaN scales past T (pad slots of them)"""
    B, Hkv, T = c.B, c.Hkv, c.T
    k_store = torch.full((B, Hkv, T + pad, c.kq.shape[-1]), 77, dtype=K.QDTYPE[c.kinds[0]], device="cuda")
    v_store = torch.full((B, Hkv, T + pad, c.vq.shape[-1]), 77, dtype=K.QDTYPE[c.kinds[1]], device="cuda")
    k_sc = torch.full((T + pad,), float("nan"), device="cuda")
    v_sc = torch.full((T + pad,), float("nan"), device="cuda")
    if T:
        k_store[:, :, :T], v_store[:, :, :T] = to_torch(c.kq), to_torch(c.vq)
        k_sc[:T], v_sc[:T] = to_torch(c.ks), to_torch(c.vs)
    return k_store, v_store, k_sc, v_sc


def _got(out, dtype):
    return A.widen(to_numpy(out), dtype)


def run_decode(K, c, step_dev_bound=None):
    """kvq_decode_attn (or kvq_decode_step_dev with the count on the device) on case c; returns float64 [B,Hq,D]."""
    d = c.dtype
    k_store, v_store, k_sc, v_sc = _stores(K, c, pad=step_dev_bound - c.T + 8 if step_dev_bound else 3)
    q = to_torch(np.ascontiguousarray(c.q[:, :, 0]), d)
    kn = None if c.kn is None else to_torch(c.kn, d)
    vn = None if c.vn is None else to_torch(c.vn, d)
    out = torch.full(q.shape, float("nan"), dtype=TD[d], device="cuda")
    if step_dev_bound:
        ws = torch.full((K.decode_attn_workspace_cap(c.B, c.Hq, c.Hkv, k_store.shape[2], c.D),), float("nan"), device="cuda")
        plan = K.DecodeStepPlan(q, k_store, k_sc, c.kinds[0], v_store, v_sc, c.kinds[1], 1e-8)
        t_dev = torch.full((1,), c.T, dtype=torch.int32, device="cuda")
        K.decode_step_dev(plan, q, kn, vn, t_dev, step_dev_bound, out, ws, c.sm)
    else:
        ws = torch.full((max(1, K.decode_attn_workspace(c.B, c.Hq, c.Hkv, c.T, c.D)),), float("nan"), device="cuda")
        K.decode_attn(q, k_store, k_sc, c.kinds[0], v_store, v_sc, c.kinds[1], c.T, out, ws, c.sm, kn, vn)
    torch.cuda.synchronize()
    return _got(out, d)


def run_extend(K, c, kn=None, vn=None):
    d = c.dtype
    k_store, v_store, k_sc, v_sc = _stores(K, c)
    q = to_torch(c.q, d)
    kn_t, vn_t = to_torch(c.kn if kn is None else kn, d), to_torch(c.vn if vn is None else vn, d)
    out = torch.full(q.shape, float("nan"), dtype=TD[d], device="cuda")
    ws = torch.full((max(1, K.extend_attn_workspace(c.B, c.Hq, c.Hkv, c.T, c.S, c.D)),), float("nan"), device="cuda")
    K.extend_attn(q, k_store, k_sc, c.kinds[0], v_store, v_sc, c.kinds[1], c.T, kn_t, vn_t, out, ws, c.sm)
    torch.cuda.synchronize()
    return _got(out, d)


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
    from efficient_llm_inference_amd import _lib
    (B, Hq, Hkv, T, D), knobs, kernel, splits = DECODE_ROUTES[route]
    for key, val in knobs.items():
        tunable(key, val)
    for c in _cases("decode", (B, Hq, Hkv, T, 1, D), splits, seed=len(route) + D):
        _lib.kernel_log_clear()
        got = run_decode(K, c)
        log = _lib.kernel_log()
        assert log[0].startswith(kernel), (route, log)
        _assert_within(c, got, qplanes=kernel.startswith("decode_attn_partial_mfma_k<8") or kernel.startswith("decode_attn_lds"),
                       what=route)
        if c.info["family"] == "outlier" and c.info["factor"] == 16.0:  # 16 x outliers: the standard tolerance holds too
            ref = c.reference()
            assert (np.abs(got - ref) <= A.TOL["f16"] * (np.abs(ref) + np.abs(ref).max())).all(), route


def test_decode_step_dev_on_the_ring_on_adversarial_inputs(K, tunable):
    """kvq_decode_step_dev with the count on the device, on the ring kernel (attn_ring_dev = 1): count 1,000 under a
    bound of 3,100 at batch 8 (the ring by size; tiles per wave derived from the count)."""
    from efficient_llm_inference_amd import _lib
    tunable("attn_ring_dev", 1)
    B, Hq, Hkv, T, D = 8, 32, 8, 1000, 128
    for fam, extra in (("sink", {}), ("probe", {}), ("vrange", {}), ("late", {})):
        c = A.make_case(fam, "decode", B, Hq, Hkv, T, 1, D, KINDS, "f16", seed=7, splits=(128, 256), probe_every=4, **extra)
        _lib.kernel_log_clear()
        got = run_decode(K, c, step_dev_bound=3100)
        log = _lib.kernel_log()
        assert log[0].startswith("decode_attn_lds_mfma_k<8, 4, 64, true, 2, 4, 128, true>") and log[1].endswith(", true>"), log
        _assert_within(c, got, qplanes=True, what="decode_step_dev ring")


EXTEND_ROUTES = {  # name -> (B, Hq, Hkv, T, S, D), expected split count
    "one split": ((1, 32, 8, 128, 16, 128), 1),
    "splits + merge": ((1, 32, 8, 1000, 16, 128), 8),
    "nq 7, splits + merge": ((1, 28, 4, 700, 9, 128), None),
    "head_dim 64, nq 3": ((2, 12, 4, 500, 7, 64), None),
}


@pytest.mark.parametrize("route", list(EXTEND_ROUTES))
def test_extend_on_adversarial_inputs(K, route):
    from efficient_llm_inference_amd import _lib
    shape, want = EXTEND_ROUTES[route]
    B, Hq, Hkv, T, S, D = shape
    _, ns, per = A.extend_plan(B, Hq, Hkv, T, S)
    assert want is None or ns == want
    variants = [None, "chunk"]  # the sink once in the store, once in the chunk
    for c in _cases("extend", shape, (per * 64,) if per else (), seed=T + S):
        for var in variants if c.info["family"] == "sink" else [None]:
            if var:
                c = A.make_case("sink", "extend", B, Hq, Hkv, T, S, D, KINDS, c.dtype, seed=T + S + 1, splits=(per * 64,), variant=var)
            _lib.kernel_log_clear()
            got = run_extend(K, c)
            log = _lib.kernel_log()
            assert log[0].startswith("extend_attn_k<") and (log[1:] == [] if ns == 1 else log[1].startswith("extend_attn_merge_k<")), log
            _assert_within(c, got, qplanes=False, what=route)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_extend_future_spike_leaves_earlier_rows_bit_identical(K, dtype):
    """A chunk token j with a huge score for every row of its kv head and a new V is in the future of rows s < j: their
    output is bit-identical to the same call without the spike; rows s >= j move to it."""
    B, Hq, Hkv, T, S, D = 1, 28, 4, 700, 9, 128
    c = A.make_case("probe", "extend", B, Hq, Hkv, T, S, D, KINDS, dtype, seed=5)
    base = run_extend(K, c)
    for j in (1, 4, S - 1):
        kn = A.widen(c.kn, dtype).astype(np.float32)
        qg = A.widen(c.q, dtype).reshape(B, Hkv, Hq // Hkv, S, D).sum(axis=(2, 3))  # [B,Hkv,D]: every row's query
        kn[:, :, j] += (40.0 / np.linalg.norm(qg, axis=-1, keepdims=True) * np.sqrt(D)) * qg
        vn = A.widen(c.vn, dtype).astype(np.float32)
        vn[:, :, j] = 8.0
        got = run_extend(K, c, kn=A.narrow(kn, dtype), vn=A.narrow(vn, dtype))
        assert np.array_equal(got[:, :, :j], base[:, :, :j]), j
        assert (np.abs(got[:, :, j:] - 8.0) < 0.1).all(), j
