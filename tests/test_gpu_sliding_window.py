"""Sliding-window attention over the quantised store on the MI355X: host-count decode (kvq_decode_attn_window /
kvq_decode_step_window), device-count decode (kvq_decode_step_dev_window, eager and graph-replayed), extend
(kvq_extend_attn_window) and the fused HF path for Mistral / Qwen2-style models. Every stored row the window excludes is
poisoned (NaN scales, extreme codes): the contract is that those rows are never read."""
import numpy as np
import pytest
import torch

from efficient_llm_inference_amd import _lib
from efficient_llm_inference_amd import kernels as K
from oracle import kvq_oracle as O
from tests import attn_ref
from tests.attn_cases import BITS
from tests.attn_ref import decode_lo, dequant
from tests.gpu_harness import got64, within_standard
from tests.util import TD

pytestmark = pytest.mark.gpu


class Store:
    """One layer's store of T tokens (+ spare slots), quantised by the oracle, with rows [0, poison) poisoned."""

    def __init__(self, B, Hkv, T, D, kinds, dtype, seed, cap=None, poison=0):
        rng = np.random.default_rng(seed)
        cap = cap or T + 4
        self.B, self.Hkv, self.T, self.D, self.kinds, self.dtype = B, Hkv, T, D, kinds, dtype
        kv = rng.standard_normal((2, B, Hkv, max(T, 1), D), dtype=np.float32).astype(np.float16)
        self.q, self.s = [], []
        self.deq = []
        for i, kind in enumerate(kinds):
            qa, _, s32 = O.quantize_tokens(kv[i][None], kind)
            qa, s32 = qa[0][:, :, :T], s32[0][:T]
            store = torch.zeros((B, Hkv, cap, K.packed_dim(kind, D)), dtype=K.QDTYPE[kind], device="cuda")
            sc = torch.ones(cap, dtype=torch.float32, device="cuda")
            if T:
                store[:, :, :T] = torch.from_numpy(qa).cuda()
                sc[:T] = torch.from_numpy(s32).cuda()
            self.deq.append(dequant(qa, s32, kind, D))
            if poison:
                store[:, :, :poison] = 127 if kind == "int8" else 0xFF  # the extreme codes
                sc[:poison] = float("nan")
            self.q.append(store)
            self.s.append(sc)

    def clone(self, poison=0):
        c = Store.__new__(Store)
        c.__dict__.update(self.__dict__)
        c.q = [t.clone() for t in self.q]
        c.s = [t.clone() for t in self.s]
        for store, sc, kind in zip(c.q, c.s, self.kinds):
            if poison:
                store[:, :, :poison] = 127 if kind == "int8" else 0xFF
                sc[:poison] = float("nan")
        return c


def _inputs(rng, shapes, dtype):
    """random GPU tensors in the compute dtype, then the float64 values they hold (what the reference must use)"""
    ts = [torch.from_numpy(rng.standard_normal(s, dtype=np.float32)).to("cuda", TD[dtype]) for s in shapes]
    return (*ts, *[got64(t) for t in ts])


def _random_store(B, Hkv, cap, D, kinds, seed):
    """A store of random codes and scales over cap slots (the device-count tests compare two kernels, not the oracle)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    st = Store.__new__(Store)
    st.kinds, st.q, st.s = kinds, [], []
    for kind in kinds:
        st.q.append(torch.randint(0, 256, (B, Hkv, cap, K.packed_dim(kind, D)), generator=g, device="cuda",
                                  dtype=torch.int32).to(torch.uint8).view(K.QDTYPE[kind]))
        st.s.append(torch.rand(cap, generator=g, device="cuda") * 0.02 + 0.002)
    return st


def _decode_ref(st, q_np, kn, vn, T, W, sm, has_new=True):
    """float64 reference: the query at position T (new token) or T - 1 over the dequantised past."""
    return attn_ref.decode(st.deq[0], st.deq[1], q_np, kn if has_new else None, vn, T, W, sm)


# (B, Hq, Hkv, D): ring TG4, ring TG1, ring hd64, one-tile MFMA, VALU hd32, VALU hd256
SHAPES = [(4, 32, 8, 128), (4, 64, 8, 128), (4, 32, 8, 64), (1, 32, 8, 128), (1, 8, 2, 32), (1, 4, 1, 256)]
KINDS = [("int8", "int8"), ("int8", "int4"), ("int4", "int4")]


def _cases():
    out = []
    for si, shape in enumerate(SHAPES):
        for ti, T in enumerate((0, 1, 63, 64, 65, 3100, 8200)):
            big = T >= 3100
            if big and (si >= 3 or (T == 8200 and si > 0)):
                continue
            kinds = KINDS[(si + ti) % 3] if not (shape[3] == 64 and shape[0] == 4) else ("int8", KINDS[ti % 3][1])
            dtype = ("f16", "bf16")[(si + ti) % 2]
            Ws = (64, T, T + 1) if big else (1, 2, 64, T, T + 1, 1 << 20)
            out.append((shape, T, kinds, dtype, tuple(w for w in Ws if w > 0)))
    return out


@pytest.mark.parametrize("shape,T,kinds,dtype,Ws", _cases())
def test_host_count_decode_window(shape, T, kinds, dtype, Ws):
    B, Hq, Hkv, D = shape
    sm = D ** -0.5
    rng = np.random.default_rng(T + D)
    q, kn_t, vn_t, q_np, kn, vn = _inputs(rng, [(B, Hq, D), (B, Hkv, D), (B, Hkv, D)], dtype)
    clean = Store(B, Hkv, T, D, kinds, dtype, seed=T)
    ws = torch.empty(K.decode_attn_workspace_cap(B, Hq, Hkv, T + 2, D), dtype=torch.float32, device="cuda")
    ref_full = torch.empty(B, Hq, D, dtype=TD[dtype], device="cuda")
    _lib.kernel_log_clear()
    K.decode_attn(q, clean.q[0], clean.s[0], kinds[0], clean.q[1], clean.s[1], kinds[1], T, ref_full, ws, sm, kn_t, vn_t)
    log_full = _lib.kernel_log()
    for W in Ws:
        for has_new in ((True, False) if T else (True,)):
            lo = decode_lo(T, W, has_new)
            st = clean.clone(poison=lo)
            out = torch.empty(B, Hq, D, dtype=TD[dtype], device="cuda")
            a = (kn_t, vn_t) if has_new else (None, None)
            _lib.kernel_log_clear()
            K.decode_attn(q, st.q[0], st.s[0], kinds[0], st.q[1], st.s[1], kinds[1], T, out, ws, sm, *a, window=W)
            torch.cuda.synchronize()
            log_w = _lib.kernel_log()
            within_standard(out, _decode_ref(clean, q_np, kn, vn, T, W, sm, has_new), dtype)
            # the same bits as the unwindowed call on the store viewed from row lo
            sl = torch.empty_like(out)
            K.decode_attn(q, st.q[0][:, :, lo:], st.s[0][lo:], kinds[0], st.q[1][:, :, lo:], st.s[1][lo:], kinds[1], T - lo,
                          sl, ws, sm, *a)
            assert torch.equal(out, sl), (W, has_new)
            if has_new and W >= T + 1:  # cuts nothing: today's call, bit for bit, same launches
                assert torch.equal(out, ref_full) and log_w == log_full, (W, log_w, log_full)
    # the step: attention as above, the new token's slot T bit-identical to the unwindowed step
    for W in (1, 64):
        lo = decode_lo(T, W)
        a, b = clean.clone(poison=lo), clean.clone()
        plan_a = K.DecodeStepPlan(q, a.q[0], a.s[0], kinds[0], a.q[1], a.s[1], kinds[1], 1e-8)
        plan_b = K.DecodeStepPlan(q, b.q[0], b.s[0], kinds[0], b.q[1], b.s[1], kinds[1], 1e-8)
        oa, ob = torch.empty_like(ref_full), torch.empty_like(ref_full)
        K.decode_step(plan_a, q, kn_t, vn_t, T, oa, ws, sm, window=W)
        K.decode_step(plan_b, q, kn_t, vn_t, T, ob, ws, sm)
        torch.cuda.synchronize()
        within_standard(oa, _decode_ref(clean, q_np, kn, vn, T, W, sm), dtype)
        for i in range(2):
            assert torch.equal(a.q[i][:, :, T], b.q[i][:, :, T]) and torch.equal(a.s[i][T], b.s[i][T])


@pytest.mark.parametrize("shape,kinds,W,fast,ring", [((1, 32, 8, 128), ("int8", "int4"), 64, 1, False),
                                                     ((1, 32, 8, 128), ("int8", "int4"), 200, 0, False),
                                                     ((16, 32, 8, 128), ("int8", "int4"), 2000, 1, True),
                                                     ((16, 32, 8, 128), ("int8", "int8"), 2000, 0, True),
                                                     ((4, 32, 8, 64), ("int8", "int8"), 130, 1, False),
                                                     ((1, 8, 2, 32), ("int4", "int4"), 40, 1, False),
                                                     ((2, 16, 4, 128), ("int8", "int8"), 1, 1, False)])
def test_device_count_decode_window(shape, kinds, W, fast, ring):
    """kvq_decode_step_dev_window against the host-count windowed step at every count of interest: 0, 1, W - 1, W,
    W + 1 and counts where the live split layout changes; the store bytes the two leave behind are identical."""
    B, Hq, Hkv, D = shape
    dtype, sm, bound = "f16", D ** -0.5, 2100
    rng = np.random.default_rng(W)
    q, kn, vn = _inputs(rng, [(B, Hq, D), (B, Hkv, D), (B, Hkv, D)], dtype)[:3]
    ws = torch.empty(K.decode_attn_workspace_cap(B, Hq, Hkv, bound + 1, D), dtype=torch.float32, device="cuda")
    base = _random_store(B, Hkv, bound + 2, D, kinds, seed=W)
    prev = _lib.get_tunable("attn_merge_fast")
    _lib.set_tunable("attn_merge_fast", fast)
    try:
        for t in sorted({0, 1, max(W - 1, 0), W, W + 1, 1000, 2047, 2048, 2049, bound}):
            lo = decode_lo(t, W)
            a = base.clone(poison=lo)
            b = a.clone()
            pa = K.DecodeStepPlan(q, a.q[0], a.s[0], kinds[0], a.q[1], a.s[1], kinds[1], 1e-8)
            pb = K.DecodeStepPlan(q, b.q[0], b.s[0], kinds[0], b.q[1], b.s[1], kinds[1], 1e-8)
            oa, ob = torch.empty_like(q), torch.empty_like(q)
            t_dev = torch.tensor([t], dtype=torch.int32, device="cuda")
            _lib.kernel_log_clear()
            K.decode_step_dev(pa, q, kn, vn, t_dev, bound, oa, ws, sm, window=W)
            log = _lib.kernel_log()
            K.decode_step(pb, q, kn, vn, t, ob, ws, sm, window=W)
            torch.cuda.synchronize()
            assert torch.isfinite(oa.float()).all(), t
            within_standard(oa, got64(ob), dtype)
            if t - lo == 0:  # nothing stored is visible: the new token's V exactly
                assert torch.allclose(oa.float(), vn.float().repeat_interleave(Hq // Hkv, 1), atol=2e-3, rtol=0)
            for i in range(2):
                assert torch.equal(a.q[i], b.q[i]) and torch.equal(a.s[i][lo:], b.s[i][lo:]), t
            if ring:  # the device-count instantiations of the ring kernel and the merge
                assert any(n.startswith("decode_attn_lds_mfma_k") and n.endswith("true>") for n in log), log
    finally:
        _lib.set_tunable("attn_merge_fast", int(prev))


def test_device_count_decode_window_graph_replay():
    """A captured decode step (kvq_decode_step_dev_window) replayed across the window boundary: every step matches the
    host-count windowed step within tolerance, and the stores stay bit-identical."""
    B, Hq, Hkv, D, W, T0, n = 2, 32, 8, 128, 48, 40, 16
    kinds, dtype, sm, bound = ("int8", "int4"), "f16", D ** -0.5, 256
    a = _random_store(B, Hkv, bound + 2, D, kinds, seed=7)
    b = a.clone()
    g = torch.Generator(device="cuda").manual_seed(3)
    q = torch.empty(B, Hq, D, dtype=torch.float16, device="cuda")
    kn = torch.empty(B, Hkv, D, dtype=torch.float16, device="cuda")
    vn = torch.empty_like(kn)
    out = torch.empty_like(q)
    ws = torch.empty(K.decode_attn_workspace_cap(B, Hq, Hkv, bound + 1, D), dtype=torch.float32, device="cuda")
    t_dev = torch.tensor([T0], dtype=torch.int32, device="cuda")
    pa = K.DecodeStepPlan(q, a.q[0], a.s[0], kinds[0], a.q[1], a.s[1], kinds[1], 1e-8)
    pb = K.DecodeStepPlan(q, b.q[0], b.s[0], kinds[0], b.q[1], b.s[1], kinds[1], 1e-8)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture (touches slot T0 of a scratch copy only)
        c = a.clone()
        pc = K.DecodeStepPlan(q, c.q[0], c.s[0], kinds[0], c.q[1], c.s[1], kinds[1], 1e-8)
        K.decode_step_dev(pc, q, kn, vn, t_dev, bound, out, ws, sm, window=W)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        K.decode_step_dev(pa, q, kn, vn, t_dev, bound, out, ws, sm, window=W)
        t_dev.add_(1)
    ob = torch.empty_like(q)
    for step in range(n):
        T = T0 + step
        q.copy_(torch.randn(B, Hq, D, generator=g, device="cuda"))
        kn.copy_(torch.randn(B, Hkv, D, generator=g, device="cuda"))
        vn.copy_(torch.randn(B, Hkv, D, generator=g, device="cuda"))
        graph.replay()
        K.decode_step(pb, q, kn, vn, T, ob, ws, sm, window=W)
        torch.cuda.synchronize()
        within_standard(out, got64(ob), dtype)
    assert int(t_dev.item()) == T0 + n
    for i in range(2):
        assert torch.equal(a.q[i], b.q[i]) and torch.equal(a.s[i], b.s[i])


EXT_CASES = [  # B, Hq, Hkv, T, S, D, W, kinds, dtype
    (1, 8, 8, 300, 16, 128, 64, ("int8", "int4"), "f16"),     # S < W, store cut
    (1, 32, 8, 500, 200, 128, 64, ("int8", "int8"), "bf16"),  # S > W: the chunk is banded
    (2, 8, 1, 0, 150, 64, 40, ("int4", "int4"), "f16"),       # T = 0, S > W
    (1, 16, 2, 1000, 40, 128, 100, ("int8", "int4"), "f16"),  # window edge inside a split
    (1, 16, 2, 1000, 40, 128, 129, ("int4", "int8"), "f16"),  # lo0 = 872: not tile aligned; edge on tile boundaries
    (1, 32, 8, 4000, 96, 128, 700, ("int8", "int4"), "bf16"), # many splits, some outside every row's window
    (1, 4, 4, 64, 8, 64, 72, ("int8", "int8"), "f16"),        # W = T + S: cuts nothing
]


@pytest.mark.parametrize("B,Hq,Hkv,T,S,D,W,kinds,dtype", EXT_CASES)
def test_extend_window(B, Hq, Hkv, T, S, D, W, kinds, dtype):
    sm = D ** -0.5
    rng = np.random.default_rng(T + S + W)
    q, knt, vnt, q_np, kn, vn = _inputs(rng, [(B, Hq, S, D), (B, Hkv, S, D), (B, Hkv, S, D)], dtype)
    lo0 = max(0, T + 1 - W)
    clean = Store(B, Hkv, T, D, kinds, dtype, seed=T)
    st = clean.clone(poison=lo0)
    kd = np.concatenate([clean.deq[0], kn.astype(np.float64)], axis=2)
    vd = np.concatenate([clean.deq[1], vn.astype(np.float64)], axis=2)
    ref = attn_ref.attention(q_np, kd, vd, T + np.arange(S), sm, W)
    ws = torch.full((max(1, K.extend_attn_workspace(B, Hq, Hkv, T, S, D)),), float("nan"), device="cuda")
    out = torch.full((B, Hq, S, D), float("nan"), dtype=TD[dtype], device="cuda")
    _lib.kernel_log_clear()
    K.extend_attn(q, st.q[0], st.s[0], kinds[0], st.q[1], st.s[1], kinds[1], T, knt, vnt, out, ws, sm, window=W)
    torch.cuda.synchronize()
    log = _lib.kernel_log()
    within_standard(out, ref, dtype)
    dt = {"f16": 0, "bf16": 1}[dtype]
    name = f"<{BITS[kinds[0]]}, {BITS[kinds[1]]}, {D}, {dt}>"
    full = torch.empty_like(out)
    _lib.kernel_log_clear()
    K.extend_attn(q, clean.q[0], clean.s[0], kinds[0], clean.q[1], clean.s[1], kinds[1], T, knt, vnt, full, ws, sm)
    log_full = _lib.kernel_log()
    assert log_full[0] == "extend_attn_k" + name
    if W >= T + S:  # today's kernels, bit for bit
        assert log == log_full and torch.equal(out, full)
    else:
        assert log[0] == "extend_attn_window_k" + name and log[1:] in ([], [f"extend_attn_merge_k<{D}, {dt}>"]), log


def test_window_zero_is_todays_call():
    B, Hq, Hkv, T, D = 1, 32, 8, 500, 128
    st = Store(B, Hkv, T, D, ("int8", "int4"), "f16", seed=1)
    q = torch.randn(B, Hq, D, dtype=torch.float16, device="cuda")
    kn = torch.randn(B, Hkv, D, dtype=torch.float16, device="cuda")
    vn = torch.randn_like(kn)
    ws = torch.empty(K.decode_attn_workspace_cap(B, Hq, Hkv, T, D), dtype=torch.float32, device="cuda")
    outs, logs = [], []
    for w in ({}, {"window": 0}):
        o = torch.empty_like(q)
        _lib.kernel_log_clear()
        K.decode_attn(q, st.q[0], st.s[0], "int8", st.q[1], st.s[1], "int4", T, o, ws, 0.1, kn, vn, **w)
        logs.append(_lib.kernel_log())
        outs.append(o)
    assert torch.equal(outs[0], outs[1]) and logs[0] == logs[1]


@pytest.mark.parametrize("arch", ["mistral-mini", "qwen2-mini"])
def test_fused_sliding_window_model_tracks_tuple_path(arch):
    """A ~100-token prompt and 48 teacher-forced tokens (the 64-token window is crossed): the fused decode's logits track
    the tuple path (HF masks the whole dequantised past), a 16-token second turn runs through the windowed extend, graph
    decode emits the eager fused tokens, and layer 0's store is the tuple path's bit for bit."""
    import efficient_llm_inference_amd as E
    from efficient_llm_inference_amd import KVCacheBenchmarker
    from efficient_llm_inference_amd.benchmarking import from_legacy_tuple, to_legacy_tuple
    from efficient_llm_inference_amd.benchmarking.offline import load_model
    from efficient_llm_inference_amd.quantization import fused_attention as FA
    from transformers.cache_utils import DynamicCache
    model, tok = load_model(arch, "cuda", torch.float16)
    n_new, n_turn = 48, 16
    with torch.no_grad():
        ids = tok("<100>", return_tensors="pt").input_ids.cuda()
        turn = tok("<16>", return_tensors="pt").input_ids.cuda()
        # a full (uncropped) prompt cache: the reference keeps every token and lets HF's mask apply the window
        out = model(input_ids=ids, use_cache=True, past_key_values=DynamicCache())
        logits = out.logits[:, -1, :]
        kv = to_legacy_tuple(out.past_key_values)
        qc = E.QuantizedKVCache(len(kv), "mixed", incremental=False)
        qc.init_from_prompt_past(kv)
        first = logits.float()
        ref_logits, toks = [], []
        for _ in range(n_new):
            nxt = torch.argmax(logits, dim=-1, keepdim=True)
            toks.append(nxt)
            out = model(input_ids=nxt, use_cache=True, past_key_values=from_legacy_tuple(qc.to_past_key_values()))
            logits = out.logits[:, -1, :]
            qc.append_from_past(to_legacy_tuple(out.past_key_values))
            ref_logits.append(logits.float())
        out = model(input_ids=turn, use_cache=True, past_key_values=from_legacy_tuple(qc.to_past_key_values()))
        ref_turn = out.logits.float()

        fc = FA.FusedQuantizedCache(len(kv), mode="mixed", reserve=ids.shape[-1] + n_new + n_turn)
        with FA.fused_attention(model, fc) as cache:
            out = model(input_ids=ids, use_cache=True, past_key_values=cache)
            assert torch.allclose(out.logits[:, -1, :].float(), first, atol=2e-2, rtol=0)  # the band-masked prompt
            worst = 0.0
            for step, nxt in enumerate(toks):
                got = model(input_ids=nxt, use_cache=True, past_key_values=cache).logits[:, -1, :].float()
                worst = max(worst, float((got - ref_logits[step]).abs().max() / ref_logits[step].abs().max()))
            assert worst < 2e-2, worst
            got = model(input_ids=turn, use_cache=True, past_key_values=cache).logits.float()
            assert float((got - ref_turn).abs().max() / ref_turn.abs().max()) < 2e-2
        T = ids.shape[-1] + n_new
        assert torch.equal(fc.qcache._k.q[0, :, :, :T], qc._k.q[0, :, :, :T])
        assert torch.equal(fc.qcache._v.q[0, :, :, :T], qc._v.q[0, :, :, :T])
        assert torch.equal(fc.qcache._k.scales[0, :T], qc._k.scales[0, :T])

    bench = KVCacheBenchmarker(model, tok, device="cuda")
    bench.fused_attention = True
    eager = bench.generate_with_quantized_kv("<100>", n_new, mode="mixed")
    bench.graph_decode = True
    graphed = bench.generate_with_quantized_kv("<100>", n_new, mode="mixed")
    assert graphed[1] == eager[1] == n_new and graphed[0] == eager[0] and graphed[2] == eager[2]


@pytest.mark.parametrize("T,S,kinds,dtype", [(300, 40, ("int8", "int4"), "f16"), (1000, 130, ("int4", "int8"), "bf16")])
def test_extend_window_kernel_equals_extend_kernel(T, S, kinds, dtype):
    """extend_attn_window_k is extend_attn_k's text with the window lines cut in. W = T + S - 1 takes the windowed kernel but hides one key
    (token 0) from the last chunk row only: every other row sees every key, and there the two kernels give the same
    bits."""
    B, Hq, Hkv, D = 1, 16, 4, 128
    rng = np.random.default_rng(T)
    q, knt, vnt = _inputs(rng, [(B, Hq, S, D), (B, Hkv, S, D), (B, Hkv, S, D)], dtype)[:3]
    st = Store(B, Hkv, T, D, kinds, dtype, seed=T)
    ws = torch.empty(max(1, K.extend_attn_workspace(B, Hq, Hkv, T, S, D)), device="cuda")
    outs, logs = [], []
    for W in (0, T + S - 1):
        out = torch.empty(B, Hq, S, D, dtype=TD[dtype], device="cuda")
        _lib.kernel_log_clear()
        K.extend_attn(q, st.q[0], st.s[0], kinds[0], st.q[1], st.s[1], kinds[1], T, knt, vnt, out, ws, D ** -0.5, window=W)
        torch.cuda.synchronize()
        outs.append(out)
        logs.append(_lib.kernel_log()[0])
    assert logs[0].startswith("extend_attn_k<") and logs[1].startswith("extend_attn_window_k<"), logs
    assert torch.equal(outs[0][:, :, :S - 1], outs[1][:, :, :S - 1])
    assert torch.isfinite(outs[1].float()).all() and not torch.equal(outs[0][:, :, S - 1], outs[1][:, :, S - 1])


@pytest.mark.parametrize("shape,kinds", [((1, 32, 8, 128), ("int8", "int4")), ((2, 16, 4, 64), ("int4", "int4")),
                                         ((1, 8, 2, 32), ("int8", "int8")), ((1, 4, 1, 256), ("int4", "int8"))])
def test_device_count_window_kernels_equal_unwindowed(shape, kinds):
    """The one-tile kernels' window instantiations (decode_attn_partial_mfma_window_k, the host-count kernel's
    text with the window lines cut in, and decode_attn_partial_window_k) with the device-count merge: on a window that cuts nothing they give the
    unwindowed device-count call's bits and store bytes."""
    B, Hq, Hkv, D = shape
    bound, t = 700, 650
    q, kn, vn = _inputs(np.random.default_rng(D), [(B, Hq, D), (B, Hkv, D), (B, Hkv, D)], "f16")[:3]
    base = _random_store(B, Hkv, bound + 2, D, kinds, seed=D)
    ws = torch.empty(K.decode_attn_workspace_cap(B, Hq, Hkv, bound + 1, D), dtype=torch.float32, device="cuda")
    t_dev = torch.tensor([t], dtype=torch.int32, device="cuda")
    outs, stores, logs = [], [], []
    for W in (0, bound + 5):
        st = base.clone()
        plan = K.DecodeStepPlan(q, st.q[0], st.s[0], kinds[0], st.q[1], st.s[1], kinds[1], 1e-8)
        out = torch.empty_like(q)
        _lib.kernel_log_clear()
        K.decode_step_dev(plan, q, kn, vn, t_dev, bound, out, ws, D ** -0.5, window=W)
        torch.cuda.synchronize()
        outs.append(out)
        stores.append(st)
        logs.append(_lib.kernel_log())
    assert "window_k" not in logs[0][0] and "window_k" in logs[1][0], logs
    assert torch.equal(outs[0], outs[1])
    for i in range(2):
        assert torch.equal(stores[0].q[i], stores[1].q[i]) and torch.equal(stores[0].s[i], stores[1].s[i])
