"""Eviction inside the quantised store on the GPU: QuantizedKVCache.keep_tokens / trim (lossless row gathers of codes and
scale words through kvq_gather_tokens), chunk_summarize (kvq_store_chunk_pool: fast and generic kernel, and the composed
route past 8,192 elements per token slice) and KVCacheBenchmarker.quant_eviction end to end. Everything is compared bit for
bit: codes and scale words against torch.index_select / the CPU model of tests/store_evict_cases.py / the GPU composition
dequantise -> chunk_summarize_kv -> quantise, dequantised pasts against the fp16 policies."""
import numpy as np
import pytest
import torch

from oracle import kvq_oracle as O
from tests import attn_ref
from tests import store_evict_cases as C
from tests.gpu_harness import K, tunable, within_standard  # noqa: F401
from tests.util import TD, to_numpy, to_torch

pytestmark = pytest.mark.gpu

MODES = ("int8", "int4", "mixed")
DTYPES = ("f16", "bf16")
KINDS = {"int8": ("int8", "int8"), "int4": ("int4", "int4"), "mixed": ("int8", "int4")}


def _past(L, B, H, T, D, dtype, seed):
    """random K/V with a different magnitude per token, as a legacy tuple on the device"""
    rng = np.random.default_rng([seed, L, B, H, T, D])
    x = rng.standard_normal((L, 2, B, H, T, D)).astype(np.float32) * np.exp2(rng.integers(-4, 3, size=(L, 2, 1, 1, T, 1))).astype(np.float32)
    t = torch.from_numpy(x).cuda().to(TD[dtype])
    return tuple((t[l, 0], t[l, 1]) for l in range(L))


def _cache(past, mode, dtype, reserve=0):
    import efficient_llm_inference_amd as E
    qc = E.QuantizedKVCache(len(past), mode, device="cuda", compute_dtype=TD[dtype])
    if reserve:
        qc.reserve(reserve)
    qc.init_from_prompt_past(past)
    return qc


def _snap(qc):
    """(K codes, K scales, V codes, V scales) of the stored tokens, cloned"""
    T = qc._k.lens[0]
    return (qc._k.q[:, :, :, :T].clone(), qc._k.scales[:, :T].clone(), qc._v.q[:, :, :, :T].clone(), qc._v.scales[:, :T].clone())


def _same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    if a.dtype.is_floating_point:
        w = torch.int32 if a.element_size() == 4 else torch.int16
        a, b = a.view(w), b.view(w)
    return a.shape == b.shape and bool(torch.equal(a, b))


def _same_past(p, r):
    return len(p) == len(r) and all(_same_bits(a, b) for x, y in zip(p, r) for a, b in zip(x, y))


# ---------------------------------------------------------------------------------------------------- gather policies

GATHER_SHAPES = [(2, 2, 3, 300, 64), (2, 1, 8, 200, 128), (1, 1, 2, 70, 32), (1, 1, 2, 40, 5)]


def _policies(T):
    from efficient_llm_inference_amd import cache as EC
    w = max(4, T // 8)
    return [
        ("sliding_window", dict(window_size=w), lambda p: EC.trim_kv_sliding_window(p, w)),
        ("prefix_window", dict(prefix_len=3, window_size=w), lambda p: EC.trim_kv_prefix_window(p, 3, w)),
        ("strided", dict(window_size=w, stride=3, prefix_len=2), lambda p: EC.trim_kv_strided(p, w, 3, 2)),
        ("block_old", dict(window_size=w, block_size=16, keep_per_block=5, prefix_len=1), lambda p: EC.trim_kv_block_old(p, w, 16, 5, 1)),
        ("budget_old", dict(window_size=w, old_budget=7, prefix_len=2), lambda p: EC.trim_kv_budget_old(p, w, 7, 2)),
    ]


def _check_gathered(qc, snap, idx, before, cap, mode, L, B, H, D, dtype, log):
    """the store after an eviction that kept tokens idx (a list; -1 = a zero row) of the snapshot"""
    n = len(idx)
    sel = torch.tensor([i if i >= 0 else 0 for i in idx], device="cuda")
    bad = torch.tensor([i < 0 for i in idx], device="cuda")
    for st, qs, ss in ((qc._k, snap[0], snap[1]), (qc._v, snap[2], snap[3])):
        assert st.lens == [n] * L and st.cap == cap and st.q.shape[3] == cap and st.scales.shape[1] == cap and st.staged == 0
        want_q = torch.index_select(qs, 3, sel)
        want_s = torch.index_select(ss, 1, sel)
        want_q[:, :, :, bad] = 0
        want_s[:, bad] = 0
        assert torch.equal(st.q[:, :, :, :n], want_q)
        assert _same_bits(st.scales[:, :n], want_s)
    assert qc.estimated_bytes() == O.estimated_bytes(mode, L, B, H, n, D, 2) == sum(l.estimated_bytes() for l in qc.layers)
    assert len(qc.layers[0]) == n and len(qc.layers[0].k_store) == n
    copy = qc.to_past_key_values(copy=True)
    if before is not None:
        assert _same_past(copy, before)
    assert _same_past(qc.to_past_key_values(), copy)  # the incremental view was reset
    Dq = [K_packed(kind, D) for kind in KINDS[mode]]
    if all(d % 16 == 0 for d in Dq):
        assert [n_.split("<")[0] for n_ in log] == ["gather_rows_k", "gather_tokens_k"], log  # code rows, then the scale table
    if all(d % 2 for d in Dq):
        assert all(n_ == "gather_tokens_k<false>" for n_ in log), log


def K_packed(kind, D):
    return D if kind == "int8" else (D + 1) // 2


def _attend_after(qc, mode, dtype, B, H, D, seed):
    """one more token through append_from_past, then one attention step over the evicted store against the float64 model"""
    rng = np.random.default_rng([seed, 9])
    L = len(qc.layers)
    new = _past(L, B, H, 1, D, dtype, seed + 1)
    qc.append_from_past(new)
    T = qc._k.lens[0]
    Hq = 2 * H
    q_np = C.to_storage(rng.standard_normal((B, Hq, D)).astype(np.float32), dtype)
    out = qc.attend(L - 1, to_torch(q_np, dtype))
    kk, vk = KINDS[mode]
    kd = attn_ref.dequant(to_numpy(qc._k.q[L - 1, :, :, :T]), to_numpy(qc._k.scales[L - 1, :T]), kk, D, dtype)
    vd = attn_ref.dequant(to_numpy(qc._v.q[L - 1, :, :, :T]), to_numpy(qc._v.scales[L - 1, :T]), vk, D, dtype)
    ref = attn_ref.decode(kd, vd, C.widen(q_np, dtype).astype(np.float64), None, None, T, 0, D ** -0.5)
    within_standard(out, ref, dtype, "attend after eviction")


@pytest.mark.parametrize("shape", GATHER_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", MODES)
def test_gather_policies(K, mode, dtype, shape):
    from efficient_llm_inference_amd import _lib
    from efficient_llm_inference_amd.cache.implementations import KEEP_INDEX_FNS
    L, B, H, T, D = shape
    past = _past(L, B, H, T, D, dtype, 3)
    runs = [(name, kw, fp16, None) for name, kw, fp16 in _policies(T)]
    runs += [("keep_tokens", None, None, list(range(T - 1, -1, -3))),                      # descending
             ("keep_tokens", None, None, [5, 5, 0, T - 1, 5, 7, 7]),                       # duplicates
             ("keep_tokens", None, None, torch.tensor([3, -1, T - 1, T, 0, 1 << 20], device="cuda")),       # out of range on the device
             ("keep_tokens", None, None, torch.tensor([2, 1, 0], dtype=torch.int32))]    # a host tensor is a list
    for name, kw, fp16, idx in runs:
        qc = _cache(past, mode, dtype, reserve=T + 9)
        cap, snap = qc._k.cap, _snap(qc)
        deq = qc.to_past_key_values(copy=True)
        qc.to_past_key_values()  # the incremental staging view holds all T tokens before the eviction
        _lib.kernel_log_clear()
        if kw is not None:
            qc.trim(name, **kw)
            log = _lib.kernel_log()
            idx_l = KEEP_INDEX_FNS[name](T, device="cuda", **kw)
            before = fp16(deq)
        else:
            qc.keep_tokens(idx)
            log = _lib.kernel_log()
            idx_l = [i if 0 <= i < T else -1 for i in (idx.tolist() if torch.is_tensor(idx) else idx)]
            before = None if -1 in idx_l else tuple((k[:, :, idx_l], v[:, :, idx_l]) for k, v in deq)
        assert idx_l is not None and 0 < len(idx_l)
        _check_gathered(qc, snap, idx_l, before, cap, mode, L, B, H, D, dtype, log)
        if D in (32, 64, 128, 256):
            _attend_after(qc, mode, dtype, B, H, D, 5)


def test_gather_no_op_and_refusals(K):
    from efficient_llm_inference_amd import _lib
    from efficient_llm_inference_amd.quantization import fused_attention as FA
    from efficient_llm_inference_amd.quantization import hf_cache
    past = _past(2, 1, 2, 20, 64, "f16", 1)
    qc = _cache(past, "mixed", "f16")
    ptrs = (qc._k.q.data_ptr(), qc._k.scales.data_ptr(), qc._v.q.data_ptr())
    _lib.kernel_log_clear()
    qc.trim("sliding_window", 64)
    qc.trim("strided", window_size=32, stride=2)
    qc.trim("sliding_window", 0)
    qc.chunk_summarize(4, 20)
    qc.chunk_summarize(4, 25)
    assert _lib.kernel_log() == [] and ptrs == (qc._k.q.data_ptr(), qc._k.scales.data_ptr(), qc._v.q.data_ptr())
    assert qc._k.lens == [20, 20]
    for bad in ([], torch.zeros(0, dtype=torch.int64, device="cuda")):
        with pytest.raises(ValueError, match="at least one token"):
            qc.keep_tokens(bad)
    for bad in ([0, 20], [-1]):
        with pytest.raises(ValueError, match="out of range"):
            qc.keep_tokens(bad)
    with pytest.raises(ValueError):
        qc.keep_tokens(torch.zeros(3, device="cuda"))
    qc.layers[1].append(past[1][0][:, :, :1], past[1][1][:, :, :1])  # one group ahead of the others
    with pytest.raises(ValueError, match="same number of tokens"):
        qc.trim("sliding_window", 4)
    with pytest.raises(ValueError, match="same number of tokens"):
        qc.chunk_summarize(4, 2)
    # a store quantised from another dtype than compute_dtype
    qb = _cache(past, "int8", "bf16")  # fp16 K/V under compute_dtype bf16
    with pytest.raises(ValueError, match="compute_dtype"):
        qb.chunk_summarize(4, 2)
    # owned by a FusedQuantizedCache whose decode graph is captured
    if FA.available():
        fc = FA.FusedQuantizedCache(2, mode="int8", reserve=32)
        fc.qcache.init_from_prompt_past(past)
        fc.t_dev = torch.zeros(1, dtype=torch.int32, device="cuda")
        for call in (lambda: fc.qcache.trim("sliding_window", 4), lambda: fc.qcache.keep_tokens([0]), lambda: fc.qcache.chunk_summarize(4, 2)):
            with pytest.raises(RuntimeError, match="captured decode graph"):
                call()
        fc.t_dev = None
        # ... or that keeps per-row key starts of a left-padded batch: they are positions in the un-evicted store
        fc.set_left_padding(torch.tensor([[0, 1, 1]], device="cuda"))  # B = 1
        snap = _snap(fc.qcache)
        _lib.kernel_log_clear()
        for call in (lambda: fc.qcache.trim("sliding_window", 4), lambda: fc.qcache.keep_tokens([0]), lambda: fc.qcache.chunk_summarize(4, 2),
                     lambda: fc.qcache.evict_by_scores(torch.ones(20, device="cuda"), 8),
                     lambda: fc.qcache.compress_prompt([past[0][0][:, :, -2:].repeat(1, 2, 1, 1)] * 2, 8),
                     lambda: fc.qcache.key_scores(0, past[0][0][:, :, -2:].repeat(1, 2, 1, 1))):
            with pytest.raises(RuntimeError, match="left-padded"):
                call()
        assert _lib.kernel_log() == [] and fc.qcache._k.lens == [20, 20] and all(_same_bits(a, b) for a, b in zip(snap, _snap(fc.qcache)))
        fc.kv_start = None
        fc.qcache.trim("sliding_window", 4)
        assert fc.qcache._k.lens == [4, 4]
    # a StagedQuantizedCache between sync() and commit()
    if hf_cache.available():
        qs = _cache(past, "int8", "f16", reserve=32)
        staged = hf_cache.StagedQuantizedCache(qs)
        cache = staged.sync()
        for i, layer in enumerate(cache.layers):
            layer.update(past[i][0][:, :, :1], past[i][1][:, :, :1])
        with pytest.raises(RuntimeError, match="in flight"):
            qs.trim("sliding_window", 4)
        staged.commit()
        qs.trim("sliding_window", 4)
        assert qs._k.lens == [4, 4] and staged.sync().layers[0].get_seq_length() == 4
        assert _same_past(tuple((l._kbuf[:, :, :4], l._vbuf[:, :, :4]) for l in staged.cache.layers), qs.to_past_key_values(copy=True))


# ---------------------------------------------------------------------------------------------------- chunk summary

SENTINEL = 0x5A


def _run_pool(K, case, fast, guard=1):
    """kvq_store_chunk_pool on a case, outputs inside sentinel-filled buffers -> (codes, scales fp32) numpy, kernel log"""
    from efficient_llm_inference_amd import _lib
    q = torch.from_numpy(case["q"]).cuda()
    s = torch.from_numpy(case["s"]).cuda()
    G, B, H, T, Dq = q.shape
    Tout = K.chunk_summary_len(T, case["chunk"], case["keep"])
    qbuf = torch.full((G, B, H, Tout + 2 * guard, Dq), SENTINEL, dtype=q.dtype, device="cuda")
    sbuf = torch.full((G, Tout + 2 * guard), -7.5, dtype=torch.float32, device="cuda")
    _lib.set_tunable("store_pool_fast", int(fast))
    _lib.kernel_log_clear()
    try:
        K.store_chunk_pool(q, s, qbuf[:, :, :, guard:guard + Tout], sbuf[:, guard:guard + Tout], case["kind"], case["D"],
                           TD[case["dtype"]], case["chunk"], case["keep"], C.EPS)
    finally:
        _lib.set_tunable("store_pool_fast", 1)
    torch.cuda.synchronize()
    log = _lib.kernel_log()
    for edge in (qbuf[:, :, :, :guard], qbuf[:, :, :, guard + Tout:]):
        assert (edge == SENTINEL).all(), "codes written outside the output rows"
    for edge in (sbuf[:, :guard], sbuf[:, guard + Tout:]):
        assert (edge == -7.5).all(), "scales written outside the output rows"
    return (to_numpy(qbuf[:, :, :, guard:guard + Tout]), to_numpy(sbuf[:, guard:guard + Tout])), log


def _composition(K, case):
    """dequantise -> chunk_summarize_kv -> quantise of the pooled rows on the GPU, raw input for the tail"""
    import efficient_llm_inference_amd as E
    q = torch.from_numpy(case["q"]).cuda()
    s = torch.from_numpy(case["s"]).cuda()
    G, B, H, T, Dq = q.shape
    kind, D, dt = case["kind"], case["D"], TD[case["dtype"]]
    keep = min(case["keep"], T)
    old = T - keep
    if old <= 0:
        return case["q"], case["s"]
    x = torch.empty(G, B, H, T, D, dtype=dt, device="cuda")
    K.dequant_tokens(q, s, x, kind)
    y = E.chunk_summarize_kv(tuple((x[g], x[g]) for g in range(G)), case["chunk"], case["keep"])
    n = y[0][0].shape[2] - keep
    pooled = torch.stack([k[:, :, :n] for k, _ in y])
    q2 = torch.empty(G, B, H, n, Dq, dtype=q.dtype, device="cuda")
    s2 = torch.empty(G, n, dtype=torch.float32, device="cuda")
    K.quant_tokens(pooled, q2, s2, torch.empty(G * n, dtype=torch.float32, device="cuda"), kind, C.EPS)
    return to_numpy(torch.cat([q2, q[:, :, :, old:]], dim=3)), to_numpy(torch.cat([s2, s[:, old:]], dim=1))


@pytest.mark.parametrize("i", range(len(C.CASES)), ids=[C.case_id(f, kw) for f, kw in C.CASES])
def test_chunk_pool_families_fast_and_generic(K, i):
    fam, kw = C.CASES[i]
    case = C.build(fam, kw)
    want = C.model(case)
    comp = _composition(K, case)
    assert not C.differs(comp, want), "GPU composition vs CPU model"
    for fast, name in ((1, "store_pool_fast_k<"), (0, "store_pool_generic_k<")):
        got, log = _run_pool(K, case, fast)
        assert len(log) == 1 and log[0].startswith(name), log
        assert got[0].shape == want[0].shape and not C.differs(got, want), (fam, kw, name)
        assert not C.differs(got, comp)


@pytest.mark.parametrize("i", range(len(C.NONFINITE_CASES)), ids=[C.case_id(f, kw) for f, kw in C.NONFINITE_CASES])
def test_chunk_pool_nonfinite_scales(K, i):
    """Tokens with a NaN or +inf scale (what the quantise kernels store for a poisoned token) inside pooled chunks and in the
    kept tail, both kernels: the summary token of such a chunk is code 0 under a NaN scale, as the composition's; the tail
    tokens move with their raw bits; the clean chunks are the model's bit for bit."""
    from tests import quant_cases as QC
    fam, kw = C.NONFINITE_CASES[i]
    case = C.build(fam, kw)
    with np.errstate(invalid="ignore", over="ignore"):
        want = C.model(case)
    T, chunk, keep = case["q"].shape[3], case["chunk"], case["keep"]
    old = T - keep
    n = (old + chunk - 1) // chunk
    poisoned = ~np.isfinite(np.add.reduceat(case["s"][:, :old], np.arange(0, old, chunk), axis=1))  # [G, n]
    assert poisoned.any() and (~poisoned).any() and np.isnan(want[1][:, :n][poisoned]).all()
    assert (np.moveaxis(want[0][:, :, :, :n], 3, 1)[poisoned].view(np.uint8) == (0x88 if case["kind"] == "int4" else 0)).all()
    for fast, name in ((1, "store_pool_fast_k<"), (0, "store_pool_generic_k<")):
        got, log = _run_pool(K, case, fast)
        assert len(log) == 1 and log[0].startswith(name), log
        assert got[0].shape == want[0].shape and np.array_equal(got[0].view(np.uint8), want[0].view(np.uint8)), (kw, name)
        assert QC.same_floats(got[1], want[1]), (kw, name, got[1], want[1])
        assert np.array_equal(got[1][:, n:].view(np.uint32), case["s"][:, old:].view(np.uint32)), "tail scale words moved raw"
        assert np.isnan(got[1][:, n:]).any() and np.isposinf(got[1][:, n:]).any()


# (B, H, D) of a token slice: 64, 1,024, exactly 8,192 elements, head_dim 256, two pieces per thread (INT8 past 256 pieces),
# and 1,536 elements: 96 INT8 pieces (256 threads, one piece each) and 48 INT4 pieces (one wave of 16-byte pieces; 32 or
# fewer take 8-byte pieces)
POOL_SHAPES = [(1, 1, 64), (1, 8, 128), (8, 8, 128), (1, 2, 256), (4, 8, 160), (2, 6, 128)]


def _pool_combos():
    """(chunk, keep, T): every chunk size with old = a multiple and a multiple + 1, old = 1, and keeps 0, 3, T - 1"""
    out = []
    for c in (1, 7, 16, 64, 100):
        out += [(c, 3, 2 * c + 3), (c, 0, 2 * c + 1 if c > 1 else 3), (c, 20, 21)]
    return out


@pytest.mark.parametrize("bhd", POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", DTYPES)
def test_chunk_summarize_shapes(K, bhd, dtype):
    from efficient_llm_inference_amd import _lib
    B, H, D = bhd
    for chunk, keep, T in _pool_combos():
        assert T <= 400
        past = _past(1, B, H, T, D, dtype, chunk)
        qc = _cache(past, "mixed", dtype, reserve=T + 5)
        cap, snap = qc._k.cap, _snap(qc)
        _lib.kernel_log_clear()
        qc.chunk_summarize(chunk, keep)
        log = _lib.kernel_log()
        assert len(log) == 2 and all(n.startswith("store_pool_fast_k<") for n in log), log  # the K store, the V store
        Tout = K.chunk_summary_len(T, chunk, keep)
        for st, qs, ss, kind in ((qc._k, snap[0], snap[1], "int8"), (qc._v, snap[2], snap[3], "int4")):
            case = dict(q=to_numpy(qs), s=to_numpy(ss), kind=kind, dtype=dtype, D=D, chunk=chunk, keep=keep)
            got = (to_numpy(st.q[:, :, :, :Tout]), to_numpy(st.scales[:, :Tout]))
            assert st.lens == [Tout] and st.cap == cap and st.staged == 0
            assert not C.differs(got, C.model(case)), (bhd, dtype, chunk, keep, T, kind)
        assert qc.estimated_bytes() == O.estimated_bytes("mixed", 1, B, H, Tout, D, 2)
        assert _same_past(qc.to_past_key_values(), qc.to_past_key_values(copy=True))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_chunk_summarize_modes_twice_and_keeps(K, mode, dtype):
    """every mode x dtype at (1, 8, 128): applied twice (the reference loop re-summarises what it summarised), keep_last T and
    T + 5 (nothing to compress), generic kernel through the tunable"""
    from efficient_llm_inference_amd import _lib
    L, B, H, T, D, chunk, keep = 2, 1, 8, 150, 128, 16, 9
    past = _past(L, B, H, T, D, dtype, 11)
    for fast in (1, 0):
        qc = _cache(past, mode, dtype)
        snap = _snap(qc)
        _lib.set_tunable("store_pool_fast", fast)
        try:
            _lib.kernel_log_clear()
            qc.chunk_summarize(chunk, keep)
            qc.chunk_summarize(chunk, keep)
            log = _lib.kernel_log()
        finally:
            _lib.set_tunable("store_pool_fast", 1)
        assert log and all(n.startswith("store_pool_fast_k<" if fast else "store_pool_generic_k<") for n in log), log
        T2 = K.chunk_summary_len(K.chunk_summary_len(T, chunk, keep), chunk, keep)
        for st, qs, ss, kind in ((qc._k, snap[0], snap[1], KINDS[mode][0]), (qc._v, snap[2], snap[3], KINDS[mode][1])):
            case = dict(q=to_numpy(qs), s=to_numpy(ss), kind=kind, dtype=dtype, D=D, chunk=chunk, keep=keep)
            assert st.lens == [T2] * L
            assert not C.differs((to_numpy(st.q[:, :, :, :T2]), to_numpy(st.scales[:, :T2])), C.model_twice(case))
    for k_all in (T, T + 5):  # the library's pure copy of T rows (the cache method does nothing there)
        case = dict(q=to_numpy(snap[0]), s=to_numpy(snap[1]), kind=KINDS[mode][0], dtype=dtype, D=D, chunk=chunk, keep=k_all)
        for fast in (1, 0):
            got, _ = _run_pool(K, case, fast)
            assert not C.differs(got, (case["q"], case["s"]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_chunk_summarize_odd_head_dim_int4(K, dtype):
    """D = 5 (three packed bytes per row, pad nibble 8): the generic kernel, whatever the tunable says"""
    from efficient_llm_inference_amd import _lib
    for chunk, keep, T in ((7, 3, 17), (16, 0, 33), (1, 2, 6)):
        past = _past(2, 1, 2, T, 5, dtype, 2)
        qc = _cache(past, "int4", dtype)
        snap = _snap(qc)
        _lib.kernel_log_clear()
        qc.chunk_summarize(chunk, keep)
        log = _lib.kernel_log()
        assert log == ["store_pool_generic_k<%d, 4>" % (0 if dtype == "f16" else 1)], log
        Tout = K.chunk_summary_len(T, chunk, keep)
        for st, qs, ss in ((qc._k, snap[0], snap[1]), (qc._v, snap[2], snap[3])):
            case = dict(q=to_numpy(qs), s=to_numpy(ss), kind="int4", dtype=dtype, D=5, chunk=chunk, keep=keep)
            got = (to_numpy(st.q[:, :, :, :Tout]), to_numpy(st.scales[:, :Tout]))
            assert not C.differs(got, C.model(case))
            n = Tout - min(keep, T)
            assert ((got[0][:, :, :, :n, 2] & 0x0F) == 8).all()  # the pad nibble of the pooled rows


@pytest.mark.parametrize("mode,dtype", [("mixed", "f16"), ("int4", "bf16"), ("int8", "bf16")])
def test_chunk_summarize_large_slice_takes_the_composition(K, mode, dtype):
    """B * H * D = 8,320: the library refuses the slice, the cache composes dequantise -> kvq_chunk_meanpool -> quantise a few
    layers at a time; same bits as the model"""
    from efficient_llm_inference_amd import _lib
    L, B, H, T, D, chunk, keep = 5, 65, 1, 45, 128, 7, 3
    past = _past(L, B, H, T, D, dtype, 4)
    qc = _cache(past, mode, dtype)
    snap = _snap(qc)
    with pytest.raises(_lib.KvqError, match="exceeds the 8192"):
        K.store_chunk_pool(snap[0], snap[1], torch.empty_like(snap[0][:, :, :, :9]), torch.empty(L, 9, device="cuda"), KINDS[mode][0],
                           D, TD[dtype], chunk, keep)
    _lib.kernel_log_clear()
    qc.chunk_summarize(chunk, keep)
    log = _lib.kernel_log()
    assert not any("store_pool" in n for n in log), log
    assert any(n.startswith("dequant_tokens") for n in log) and any(n.startswith("chunk_pool_") for n in log) and \
        any(n.startswith("quant_") for n in log), log
    Tout = K.chunk_summary_len(T, chunk, keep)
    for st, qs, ss, kind in ((qc._k, snap[0], snap[1], KINDS[mode][0]), (qc._v, snap[2], snap[3], KINDS[mode][1])):
        case = dict(q=to_numpy(qs), s=to_numpy(ss), kind=kind, dtype=dtype, D=D, chunk=chunk, keep=keep)
        assert st.lens == [Tout] * L
        assert not C.differs((to_numpy(st.q[:, :, :, :Tout]), to_numpy(st.scales[:, :Tout])), C.model(case))


# ---------------------------------------------------------------------------------------------------- end to end

class _PastRecorder:
    """the model as the benchmarker calls it, keeping a copy of the past handed to every forward"""

    def __init__(self, model, to_legacy):
        self.__dict__.update(m=model, pasts=[], to_legacy=to_legacy)

    def __getattr__(self, name):
        return getattr(self.__dict__["m"], name)

    def __call__(self, *a, **kw):
        past = kw.get("past_key_values")
        if past is not None:
            self.pasts.append(tuple((k.clone(), v.clone()) for k, v in self.to_legacy(past)))
        return self.__dict__["m"](*a, **kw)


def _qdq(kv, mode):
    """quantise -> dequantise of a legacy tuple, token by token (every token has its own scale)"""
    return _cache(kv, mode, "f16").to_past_key_values(copy=True)


@pytest.mark.parametrize("policy", ["strided", "chunk_summary"])
def test_benchmarker_quant_eviction(K, policy):
    import efficient_llm_inference_amd as E
    from efficient_llm_inference_amd import KVCacheBenchmarker
    from efficient_llm_inference_amd import cache as EC
    from efficient_llm_inference_amd.benchmarking import from_legacy_tuple, to_legacy_tuple
    from efficient_llm_inference_amd.benchmarking.offline import load_model
    model, tok = load_model("llama-mini", "cuda", torch.float16)
    rec = _PastRecorder(model, to_legacy_tuple)
    bench = KVCacheBenchmarker(rec, tok, device="cuda")
    n_new, mode = 6, "mixed"
    if policy == "strided":
        kw = dict(window_size=16, stride=3, prefix_len=2)
        fp16 = lambda p: EC.trim_kv_strided(p, 16, 3, 2)
    else:
        kw = dict(chunk_size=16, keep_last=8)

        def fp16(p):  # the fp16 policy, its pooled rows requantised (the store holds them quantised), the tail untouched
            y = E.chunk_summarize_kv(p, 16, 8)
            n = y[0][0].shape[2] - min(8, p[0][0].shape[2])
            if y[0][0] is p[0][0] or n <= 0:
                return p
            head = _qdq(tuple((k[:, :, :n], v[:, :, :n]) for k, v in y), mode)
            return tuple((torch.cat([hk, k[:, :, n:]], 2), torch.cat([hv, v[:, :, n:]], 2)) for (hk, hv), (k, v) in zip(head, y))
    bench.quant_eviction = (policy, kw)
    text, got_new, mbytes = bench.generate_with_quantized_kv("<70>", n_new, mode=mode)
    assert got_new == n_new and len(rec.pasts) == n_new
    # the same decode written out: dequantised store -> fp16 policy after every appended token
    with torch.no_grad():
        ids = tok("<70>", return_tensors="pt").input_ids.cuda()
        out = model(input_ids=ids, use_cache=True)
        shadow = _qdq(to_legacy_tuple(out.past_key_values), mode)
        logits, gen = out.logits[:, -1, :], ids.clone()
        for step in range(n_new):
            nxt = torch.argmax(logits, dim=-1, keepdim=True)
            gen = torch.cat([gen, nxt], dim=-1)
            assert _same_past(rec.pasts[step], shadow), step
            out = model(input_ids=nxt, use_cache=True, past_key_values=from_legacy_tuple(tuple((k.clone(), v.clone()) for k, v in shadow)))
            logits = out.logits[:, -1, :]
            new = _qdq(tuple((k[:, :, -1:], v[:, :, -1:]) for k, v in to_legacy_tuple(out.past_key_values)), mode)
            shadow = fp16(tuple((torch.cat([k, nk], 2), torch.cat([v, nv], 2)) for (k, v), (nk, nv) in zip(shadow, new)))
    assert text == tok.decode(gen[0], skip_special_tokens=True)
    qc = bench._last_qcache
    assert _same_past(qc.to_past_key_values(copy=True), shadow)
    assert qc._k.lens[0] < 70 and mbytes == qc.estimated_bytes() / (1024 ** 2)
    for flags in (dict(fused_attention=True), dict(fused_attention=True, graph_decode=True)):
        b2 = KVCacheBenchmarker(model, tok, device="cuda")
        b2.quant_eviction = (policy, kw)
        for k_, v_ in flags.items():
            setattr(b2, k_, v_)
        with pytest.raises(RuntimeError, match="quant_eviction does not combine"):
            b2.generate_with_quantized_kv("<70>", 2, mode=mode)


def test_integration_doc_store_eviction_sequence(K):
    """INTEGRATION.md's Level-2 store-eviction block, executed: kvq_store_chunk_pool, then the two reinterpreted gathers"""
    import ctypes
    import os
    import re

    from efficient_llm_inference_amd import _lib
    from tests.conftest import ROOT
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    src = [b for b in re.findall(r"```python\n(.*?)```", text, flags=re.S) if "kvq_store_chunk_pool" in b]
    assert len(src) == 1
    L, B, H, T, D = 2, 1, 4, 45, 64
    qc = _cache(_past(L, B, H, T, D, "f16", 8), "int8", "f16")
    store, scales = qc._k.q, qc._k.scales
    Tcap = qc._k.cap
    ns = {"ctypes": ctypes, "torch": torch, "lib": _lib.load(), "KvqDims": _lib.KvqDims, "KvqStrides": _lib.KvqStrides, "byref": ctypes.byref,
          "KVQ_F16": 0, "store": store, "scales": scales, "Tcap": Tcap, "L": L, "B": B, "H": H, "T": T, "D": D,
          "store_st": _lib.KvqStrides(*store.stride()[:4]), "store2": torch.full_like(store, SENTINEL),
          "scales2": torch.zeros_like(scales), "stream": ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)}
    exec(compile(src[0], "INTEGRATION.md[Level 2, store eviction]", "exec"), ns)
    torch.cuda.synchronize()
    case = dict(q=to_numpy(store[:, :, :, :T]), s=to_numpy(scales[:, :T]), kind="int8", dtype="f16", D=D, chunk=16, keep=8)
    want = C.model(case)
    Tout = ns["Tout"]
    assert not C.differs((to_numpy(ns["store2"][:, :, :, :Tout]), to_numpy(ns["scales2"][:, :Tout])), want)
    assert (ns["store2"][:, :, :, Tout:] == SENTINEL).all()
    n = ns["idx"].numel()
    assert not C.differs((to_numpy(ns["store3"][:, :, :, :n]), to_numpy(ns["scales3"][:, :n])), (want[0][:, :, :, ::2], want[1][:, ::2]))
