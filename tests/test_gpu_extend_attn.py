"""Multi-token causal attention straight from the INT8 / packed-INT4 store (kvq_extend_attn) on the MI355X: the kernel
against a float64 restatement of the reference pipeline (dequantise the stored tokens, cat the chunk's exact K/V,
softmax(q K^T) V under HF's lower-right-aligned causal mask), the cache method that builds a store chunk by chunk,
and a multi-token forward of a model through ``fused_attention``.

Floating point: same tolerances as the decode kernel (tests/test_gpu_attn.py): the kernel accumulates exact integer x
fp16 / bf16 products in fp32, skips the reference's rounding of the dequantised values and rounds P to the compute
dtype for the matrix cores."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

from efficient_llm_inference_amd import _lib
from oracle import kvq_oracle as O
from tests.attn_cases import TOL, Case, bound, extend_plan, narrow
from tests.attn_cases import check as budget_check
from tests.gpu_harness import K, got64, rand_like, within_standard  # noqa: F401
from tests.util import TD, to_torch

pytestmark = pytest.mark.gpu

KINDS = [("int8", "int8"), ("int8", "int4"), ("int4", "int4"), ("int4", "int8")]


def _as_f32(a, dtype):
    return O.bf16_bits_to_f32(a) if dtype == "bf16" else a.astype(np.float32)


def _hf_layout(x_np, dtype):
    """[B, H, S, D] numpy -> a [B, H, S, D] view of a [B, S, H, D] tensor (HF's projection layout)."""
    return to_torch(np.ascontiguousarray(x_np.transpose(0, 2, 1, 3)), dtype).transpose(1, 2)


def _case(K, B, Hq, Hkv, T, S, D, k_kind, v_kind, dtype, strided, tcap_pad=5):
    rng = np.random.default_rng(zlib.crc32(repr((B, Hq, Hkv, T, S, D, k_kind, v_kind, dtype)).encode()))
    kv = [rand_like((1, B, Hkv, T, D), dtype, rng), rand_like((1, B, Hkv, T, D), dtype, rng)]
    if T:  # outlier channel in K, as real keys have
        k32 = _as_f32(kv[0], dtype)
        k32[..., 3] *= 6.0
        kv[0] = narrow(k32, dtype)
    odt = "bf16" if dtype == "bf16" else None
    kq, _, ks = O.quantize_tokens(kv[0], k_kind, dtype=odt)
    vq, _, vs = O.quantize_tokens(kv[1], v_kind, dtype=odt)
    q_np = rand_like((B, Hq, S, D), dtype, rng)
    kn_np = rand_like((B, Hkv, S, D), dtype, rng)
    vn_np = rand_like((B, Hkv, S, D), dtype, rng)
    sm = D ** -0.5
    ref = O.extend_attention(_as_f32(q_np, dtype), kq[0], ks[0], k_kind, vq[0], vs[0], v_kind, D, sm,
                           _as_f32(kn_np, dtype), _as_f32(vn_np, dtype), kv_dtype=dtype)

    Tcap = T + tcap_pad
    k_store = torch.zeros(B, Hkv, Tcap, kq.shape[-1], dtype=K.QDTYPE[k_kind], device="cuda")
    v_store = torch.zeros(B, Hkv, Tcap, vq.shape[-1], dtype=K.QDTYPE[v_kind], device="cuda")
    k_sc = torch.full((Tcap,), float("nan"), device="cuda")
    v_sc = torch.full((Tcap,), float("nan"), device="cuda")
    if T:
        k_store[:, :, :T] = to_torch(kq[0])
        v_store[:, :, :T] = to_torch(vq[0])
        k_sc[:T] = to_torch(ks[0])
        v_sc[:T] = to_torch(vs[0])
    # guard tokens past T: garbage codes and NaN scales that must never reach the result
    k_store[:, :, T:] = 77 if k_kind == "int8" else 0x7F
    v_store[:, :, T:] = 77 if v_kind == "int8" else 0x7F
    if strided:
        q, kn, vn = _hf_layout(q_np, dtype), _hf_layout(kn_np, dtype), _hf_layout(vn_np, dtype)
        out = torch.full((B, S, Hq, D), float("nan"), dtype=TD[dtype], device="cuda").transpose(1, 2)
    else:
        q, kn, vn = to_torch(q_np, dtype), to_torch(kn_np, dtype), to_torch(vn_np, dtype)
        out = torch.full((B, Hq, S, D), float("nan"), dtype=TD[dtype], device="cuda")
    ws = torch.full((max(1, K.extend_attn_workspace(B, Hq, Hkv, T, S, D)),), float("nan"), device="cuda")
    _lib.kernel_log_clear()
    K.extend_attn(q, k_store, k_sc, k_kind, v_store, v_sc, v_kind, T, kn, vn, out, ws, sm)
    torch.cuda.synchronize()
    within_standard(out, ref, dtype)
    # and the error budget of tests/attn_cases.py on top (per output row: stricter than the tolerance where a row's
    # outputs are small against the tensor's largest)
    c = Case("extend", dtype, (k_kind, v_kind), sm, q_np, kv[0][0], kv[1][0], kn_np, vn_np, {})
    ok, worst = budget_check(got64(out), ref, bound(c, ref))
    assert ok, worst
    _check_launches(B, Hq, Hkv, T, S, D, k_kind, v_kind, dtype)


def _check_launches(B, Hq, Hkv, T, S, D, k_kind, v_kind, dtype):
    """The launches that ran: extend_attn_k alone for one split, followed by extend_attn_merge_k for several."""
    dt = {"f16": 0, "bf16": 1}[dtype]
    bits = {"int8": 8, "int4": 4}
    want = [f"extend_attn_k<{bits[k_kind]}, {bits[v_kind]}, {D}, {dt}>"]
    if extend_plan(B, Hq, Hkv, T, S)[1] > 1:
        want.append(f"extend_attn_merge_k<{D}, {dt}>")
    assert _lib.kernel_log() == want, (_lib.kernel_log(), want)


CASES = [  # B, Hq, Hkv, T, S, D
    (1, 8, 8, 0, 17, 64),        # empty store: plain causal attention over the chunk
    (3, 4, 1, 1, 5, 128),        # one stored token, multi-query
    (1, 32, 8, 63, 16, 128),     # Llama-3-8B grouping, a ragged stored tile
    (2, 16, 2, 64, 2, 64),       # 8 per kv head, exactly one stored tile
    (1, 16, 1, 1000, 200, 128),  # 16 per kv head, 50 query blocks, causal tiles of the chunk
    (1, 8, 2, 5000, 1, 128),     # S = 1, several splits
    (3, 8, 8, 1000, 17, 64),     # one query head per kv head
    (1, 32, 8, 5000, 16, 128),   # speculative verify: split stored tokens + merge
]
EDGE_CASES = [  # block, wave, tile and split edges; tests/test_attn_discrimination.py runs its families at these shapes
    (1, 21, 7, 300, 5, 128),     # 3 query heads per kv head: block and wave edges inside a chunk position's heads
    (1, 10, 2, 200, 13, 64),     # 5 per kv head, S * nq = 65: one row into a second query block
    (2, 12, 2, 500, 11, 64),     # 6 per kv head (Qwen2-1.5B grouping), S * nq = 66
    (1, 28, 4, 700, 9, 128),     # 7 per kv head (Qwen2.5-7B grouping), S * nq = 63
    (1, 24, 2, 300, 16, 128),    # 12 per kv head: 192 rows, every wave edge inside a position
    (1, 16, 2, 130, 8, 128),     # S * nq = 64: exactly one query block
    (1, 8, 4, 100, 64, 64),      # S = 64: one whole chunk tile
    (1, 4, 4, 129, 65, 128),     # S = 65: a second chunk tile of one token
    (1, 32, 8, 319, 16, 128),    # T = 64 k - 1, 3 splits of 2 tiles: a last split of one ragged tile
    (1, 32, 8, 320, 16, 128),    # T = 64 k: a last split of one tile
    (1, 32, 8, 321, 16, 128),    # T = 64 k + 1: 3 splits of 2 tiles, the last tile one token
    (1, 32, 2, 12288, 4, 128),   # the 64-split cap binds: 192 tiles, 96 splits by tiles, 512 by target
]
CASES += EDGE_CASES


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("kinds", KINDS)
def test_extend_attn_matches_oracle(K, case, kinds):
    for dtype in ("f16", "bf16"):
        _case(K, *case, kinds[0], kinds[1], dtype, strided=CASES.index(case) % 2 == 1)


def test_extend_attn_single_token_agrees_with_decode_attn(K):
    """S = 1 is a decode step with the new token given: the two kernels agree within the tolerance."""
    rng = np.random.default_rng(11)
    B, Hq, Hkv, T, D = 2, 32, 8, 3000, 128
    kv = rng.standard_normal((2, 1, B, Hkv, T, D)).astype(np.float16)
    kq, _, ks = O.quantize_tokens(kv[0], "int8")
    vq, _, vs = O.quantize_tokens(kv[1], "int4")
    k_store, v_store = to_torch(kq[0]), to_torch(vq[0])
    k_sc, v_sc = to_torch(ks[0]), to_torch(vs[0])
    q = torch.from_numpy(rng.standard_normal((B, Hq, 1, D)).astype(np.float16)).cuda()
    kn = torch.from_numpy(rng.standard_normal((B, Hkv, 1, D)).astype(np.float16)).cuda()
    vn = torch.from_numpy(rng.standard_normal((B, Hkv, 1, D)).astype(np.float16)).cuda()
    out_e = torch.empty(B, Hq, 1, D, dtype=torch.float16, device="cuda")
    out_d = torch.empty(B, Hq, D, dtype=torch.float16, device="cuda")
    ws_e = torch.empty(max(1, K.extend_attn_workspace(B, Hq, Hkv, T, 1, D)), device="cuda")
    ws_d = torch.empty(K.decode_attn_workspace(B, Hq, Hkv, T, D), device="cuda")
    K.extend_attn(q, k_store, k_sc, "int8", v_store, v_sc, "int4", T, kn, vn, out_e, ws_e, D ** -0.5)
    K.decode_attn(q[:, :, 0], k_store, k_sc, "int8", v_store, v_sc, "int4", T, out_d, ws_d, D ** -0.5, kn[:, :, 0], vn[:, :, 0])
    torch.cuda.synchronize()
    a, b = out_e[:, :, 0].double(), out_d.double()
    assert ((a - b).abs() <= TOL["f16"] * (b.abs() + b.abs().max())).all(), float((a - b).abs().max())


def _quantized_prefix(x, kind):
    """O.quantize_tokens of [1,B,H,t,D] that also takes t = 0: (q [1,B,H,t,Dq], scales_f32 [1,t])."""
    if x.shape[3] == 0:
        Dq = x.shape[4] if kind == "int8" else (x.shape[4] + 1) // 2
        return np.zeros(x.shape[:4] + (Dq,), np.int8 if kind == "int8" else np.uint8), np.zeros((1, 0), np.float32)
    q, _, s32 = O.quantize_tokens(x, kind)
    return q, s32


@pytest.mark.parametrize("mode", ["mixed", "int4"])
def test_cache_extend_chunked_equals_whole(mode):
    """QuantizedKVCache.extend(append=True) chunk by chunk: every chunk's output matches the oracle over what was
    stored before it, and the final store is bit-identical to init_from_prompt_past on the whole sequence."""
    import efficient_llm_inference_amd as E
    kk, vk = {"mixed": ("int8", "int4"), "int4": ("int4", "int4")}[mode]
    L, B, Hq, Hkv, D = 2, 1, 8, 2, 128
    chunks = [37, 64, 1, 200]
    N = sum(chunks)
    rng = np.random.default_rng(3)
    kv = rng.standard_normal((L, 2, B, Hkv, N, D)).astype(np.float16)
    qs = rng.standard_normal((L, B, Hq, N, D)).astype(np.float16)
    kv_t = torch.from_numpy(kv).cuda()
    q_t = torch.from_numpy(qs).cuda()
    qc = E.QuantizedKVCache(L, mode)
    t0 = 0
    for S in chunks:
        for l in range(L):
            kq, ks = _quantized_prefix(kv[l:l + 1, 0, :, :, :t0], kk)
            vq, vs = _quantized_prefix(kv[l:l + 1, 1, :, :, :t0], vk)
            ref = O.extend_attention(qs[l, :, :, t0:t0 + S].astype(np.float32), kq[0], ks[0], kk, vq[0], vs[0], vk, D, D ** -0.5,
                                   kv[l, 0, :, :, t0:t0 + S].astype(np.float32), kv[l, 1, :, :, t0:t0 + S].astype(np.float32))
            out = qc.extend(l, q_t[l, :, :, t0:t0 + S], kv_t[l, 0, :, :, t0:t0 + S], kv_t[l, 1, :, :, t0:t0 + S])
            torch.cuda.synchronize()
            within_standard(out, ref, "f16")
        t0 += S
    whole = E.QuantizedKVCache(L, mode)
    whole.init_from_prompt_past(tuple((kv_t[l, 0], kv_t[l, 1]) for l in range(L)))
    for a, b in ((qc._k, whole._k), (qc._v, whole._v)):
        assert a.lens == b.lens == [N] * L
        assert torch.equal(a.q[:, :, :, :N], b.q[:, :, :, :N])
        assert torch.equal(a.scales[:, :N], b.scales[:, :N])


@pytest.mark.parametrize("name", ["llama-mini", "gpt2-mini"])
def test_fused_multi_token_forward_tracks_tuple_path(name):
    """A prompt through fused_attention, then ONE forward of 24 continuation tokens into the non-empty quantised
    cache (kvq_extend_attn): the logits at every position track the tuple path (dequantised past handed to HF), layer
    0's store is what quantising the whole sequence writes, and decoding continues."""
    import efficient_llm_inference_amd as E
    from efficient_llm_inference_amd.benchmarking import from_legacy_tuple, to_legacy_tuple
    from efficient_llm_inference_amd.benchmarking.offline import load_model
    from efficient_llm_inference_amd.quantization import fused_attention as FA
    model, tok = load_model(name, "cuda", torch.float16)
    mode, n = "mixed", 24
    with torch.no_grad():
        ids = tok("<120>", return_tensors="pt").input_ids.cuda()
        P = ids.shape[-1]
        cont = torch.randint(0, model.config.vocab_size, (1, n), generator=torch.Generator().manual_seed(1)).cuda()
        kv = to_legacy_tuple(model(input_ids=ids, use_cache=True).past_key_values)
        L = len(kv)
        qc = E.QuantizedKVCache(L, mode, incremental=False)
        qc.init_from_prompt_past(kv)
        ref_out = model(input_ids=cont, use_cache=True, past_key_values=from_legacy_tuple(qc.to_past_key_values()))
        ref = ref_out.logits.float()
        ref_kv = to_legacy_tuple(ref_out.past_key_values)

        fc = FA.FusedQuantizedCache(L, mode=mode, reserve=P + n + 1)
        with FA.fused_attention(model, fc) as cache:
            model(input_ids=ids, use_cache=True, past_key_values=cache)
            got = model(input_ids=cont, use_cache=True, past_key_values=cache).logits.float()
        assert got.shape == ref.shape == (1, n, model.config.vocab_size)
        worst = float(((got - ref).abs().amax(dim=-1) / ref.abs().amax(dim=-1)).max())
        assert worst < 2e-2, worst
        assert cache.get_seq_length() == P + n and fc.qcache._k.lens == [P + n] * L
        # layer 0's K/V of the continuation depend on the embeddings only: the same bits in both paths
        whole = E.QuantizedKVCache(1, mode)
        whole.init_from_prompt_past(((torch.cat([kv[0][0], ref_kv[0][0][:, :, P:]], 2),
                                      torch.cat([kv[0][1], ref_kv[0][1][:, :, P:]], 2)),))
        for a, b in ((fc.qcache._k, whole._k), (fc.qcache._v, whole._v)):
            assert torch.equal(a.q[0, :, :, :P + n], b.q[0, :, :, :P + n])
            assert torch.equal(a.scales[0, :P + n], b.scales[0, :P + n])
        # decoding continues: one step against the tuple path over the fused cache's own store
        nxt = torch.argmax(got[:, -1:], dim=-1)
        want = model(input_ids=nxt, use_cache=True,
                     past_key_values=from_legacy_tuple(fc.qcache.to_past_key_values(copy=True))).logits[:, -1].float()
        with FA.fused_attention(model, fc) as cache:
            step = model(input_ids=nxt, use_cache=True, past_key_values=cache).logits[:, -1].float()
        assert float((step - want).abs().max() / want.abs().max()) < 2e-2
        assert cache.get_seq_length() == P + n + 1

        # a padding mask and graph mode are refused for a multi-token forward
        fc2 = FA.FusedQuantizedCache(L, mode=mode, reserve=P + n)
        with FA.fused_attention(model, fc2) as cache:
            model(input_ids=ids, use_cache=True, past_key_values=cache)
            mask = torch.ones(1, P + n, dtype=torch.long, device="cuda")
            mask[0, 0] = 0
            with pytest.raises(RuntimeError, match="padding mask"):
                model(input_ids=cont, attention_mask=mask, use_cache=True, past_key_values=cache)
        fc3 = FA.FusedQuantizedCache(L, mode=mode, reserve=P + n)
        with FA.fused_attention(model, fc3) as cache:
            model(input_ids=ids, use_cache=True, past_key_values=cache)
            fc3.t_dev = torch.full((1,), P, dtype=torch.int32, device="cuda")
            with pytest.raises(RuntimeError, match="graph mode"):
                model(input_ids=cont, use_cache=True, past_key_values=cache)
        assert fc3.qcache._k.lens == [P] * L  # refused before anything was appended


@pytest.mark.parametrize("B,T,S,dtype", [(8, 16384, 16, "f16"), (8, 16384, 16, "bf16"), (1, 16384, 512, "f16")])
def test_extend_attn_full_size_against_float64_attention_on_the_device(K, B, T, S, dtype):
    """The two measured extend shapes (speculative verify at B 8 x T 16,384 x S 16, chunked prefill at B 1 x
    T 16,384 x S 512; Llama-3-8B heads, INT8 K + INT4 V) against an independent computation: the stores dequantised by
    the token-table kernel (bit-exact with the reference), then float64 softmax(q K^T) V with torch ops on the GPU under
    the lower-right causal mask, one (batch row, kv head) at a time. Same tolerance as the small-shape oracle tests."""
    Hq, Hkv, D = 32, 8, 128
    nq, td = Hq // Hkv, TD[dtype]
    g = torch.Generator(device="cuda").manual_seed(T + S + B)
    k_store = torch.randint(-127, 128, (B, Hkv, T, D), dtype=torch.int8, device="cuda", generator=g)
    v_store = torch.randint(0, 256, (B, Hkv, T, D // 2), dtype=torch.uint8, device="cuda", generator=g)
    k_sc = (10.0 ** (torch.rand(T, device="cuda", generator=g) - 1.0)) * (4.0 / 127.0)
    v_sc = (torch.rand(T, device="cuda", generator=g) * 0.9 + 0.1) * (3.0 / 7.0)
    k_sc, v_sc = k_sc.to(td).float(), v_sc.to(td).float()  # stored scales are compute-dtype values
    q = torch.randn(B, Hq, S, D, device="cuda", generator=g).to(td)
    kn = torch.randn(B, Hkv, S, D, device="cuda", generator=g).to(td)
    vn = torch.randn(B, Hkv, S, D, device="cuda", generator=g).to(td)
    sm = D ** -0.5
    out = torch.full((B, Hq, S, D), float("nan"), dtype=td, device="cuda")
    ws = torch.full((max(1, K.extend_attn_workspace(B, Hq, Hkv, T, S, D)),), float("nan"), device="cuda")
    _lib.kernel_log_clear()
    K.extend_attn(q, k_store, k_sc, "int8", v_store, v_sc, "int4", T, kn, vn, out, ws, sm)
    torch.cuda.synchronize()
    _check_launches(B, Hq, Hkv, T, S, D, "int8", "int4", dtype)

    kd = torch.empty(1, B, Hkv, T, D, dtype=td, device="cuda")
    vd = torch.empty(1, B, Hkv, T, D, dtype=td, device="cuda")
    K.dequant_tokens(k_store.unsqueeze(0), k_sc.unsqueeze(0), kd, "int8")
    K.dequant_tokens(v_store.unsqueeze(0), v_sc.unsqueeze(0), vd, "int4")
    future = torch.arange(S, device="cuda")[None, :] > torch.arange(S, device="cuda")[:, None]  # [s, j]
    ref = torch.empty(B, Hq, S, D, dtype=torch.float64, device="cuda")
    for b in range(B):
        for h in range(Hkv):
            kf = torch.cat([kd[0, b, h], kn[b, h]]).double()  # [T + S, D]
            vf = torch.cat([vd[0, b, h], vn[b, h]]).double()
            sc = torch.einsum("hsd,td->hst", q[b, h * nq:(h + 1) * nq].double(), kf) * sm
            sc[:, :, T:].masked_fill_(future, float("-inf"))
            ref[b, h * nq:(h + 1) * nq] = torch.einsum("hst,td->hsd", torch.softmax(sc, dim=-1), vf)
            del kf, vf, sc
    got = out.double()
    assert torch.isfinite(got).all()
    bound = TOL[dtype] * (ref.abs() + ref.abs().max())
    assert bool(((got - ref).abs() <= bound).all()), float(((got - ref).abs() / bound).max())


def test_fused_multi_token_forward_seven_query_heads_per_kv_head():
    """fused_attention's multi-token forward on a random-init Llama with 14 query heads on 2 kv heads at head_dim 64
    (7 per kv head: query blocks and waves end inside a chunk position's heads): 24 continuation tokens into a non-empty
    quantised cache track the tuple path (dequantised past handed to HF), through kvq_extend_attn."""
    import efficient_llm_inference_amd as E
    from transformers import LlamaConfig, LlamaForCausalLM
    from efficient_llm_inference_amd.benchmarking import from_legacy_tuple, to_legacy_tuple
    from efficient_llm_inference_amd.quantization import fused_attention as FA
    torch.manual_seed(7)
    cfg = LlamaConfig(hidden_size=896, intermediate_size=1536, num_hidden_layers=2, num_attention_heads=14,
                      num_key_value_heads=2, head_dim=64, vocab_size=260, max_position_embeddings=2048, bos_token_id=0,
                      eos_token_id=256, pad_token_id=None, tie_word_embeddings=False)
    model = LlamaForCausalLM(cfg).to(device="cuda", dtype=torch.float16).eval()
    gen = torch.Generator().manual_seed(3)
    P, n = 150, 24
    ids = torch.randint(0, cfg.vocab_size, (1, P), generator=gen).cuda()
    cont = torch.randint(0, cfg.vocab_size, (1, n), generator=gen).cuda()
    with torch.no_grad():
        kv = to_legacy_tuple(model(input_ids=ids, use_cache=True).past_key_values)
        L = len(kv)
        qc = E.QuantizedKVCache(L, "mixed", incremental=False)
        qc.init_from_prompt_past(kv)
        ref = model(input_ids=cont, use_cache=True, past_key_values=from_legacy_tuple(qc.to_past_key_values())).logits.float()
        fc = FA.FusedQuantizedCache(L, mode="mixed", reserve=P + n + 1)
        with FA.fused_attention(model, fc) as cache:
            model(input_ids=ids, use_cache=True, past_key_values=cache)
            torch.cuda.synchronize()
            _lib.kernel_log_clear()
            got = model(input_ids=cont, use_cache=True, past_key_values=cache).logits.float()
            torch.cuda.synchronize()
            log = _lib.kernel_log()
    assert "extend_attn_k<8, 4, 64, 0>" in log, log
    assert got.shape == ref.shape == (1, n, cfg.vocab_size)
    worst = float(((got - ref).abs().amax(dim=-1) / ref.abs().amax(dim=-1)).max())
    assert worst < 2e-2, worst
    assert cache.get_seq_length() == P + n


def test_extend_attn_refusals(K):
    """Unsupported head_dim, an empty chunk and mismatched shapes raise before any launch."""
    from efficient_llm_inference_amd import _lib
    dev = "cuda"

    def args(B=1, Hq=4, Hkv=2, T=10, S=3, D=128, kn_S=None, q_dtype=torch.float16):
        q = torch.zeros(B, Hq, S, D, dtype=q_dtype, device=dev)
        ks = torch.zeros(B, Hkv, T + 1, D, dtype=torch.int8, device=dev)
        vs = torch.zeros(B, Hkv, T + 1, D, dtype=torch.int8, device=dev)
        sc = torch.ones(T + 1, device=dev)
        kn = torch.zeros(B, Hkv, S if kn_S is None else kn_S, D, dtype=torch.float16, device=dev)
        out = torch.zeros_like(q)
        ws = torch.zeros(1 << 16, device=dev)
        return (q, ks, sc, "int8", vs, sc, "int8", T, kn, kn.clone(), out, ws, 0.1)

    torch.cuda.synchronize()
    _lib.load().kvq_kernel_log_clear()
    for D in (32, 256, 80, 96):
        with pytest.raises(_lib.KvqError, match="head_dim"):
            K.extend_attn(*args(D=D))
        with pytest.raises(_lib.KvqError, match="dims"):
            K.extend_attn_workspace(1, 4, 2, 10, 3, D)
    with pytest.raises(_lib.KvqError, match="S >= 1"):
        K.extend_attn(*args(S=0))
    with pytest.raises(_lib.KvqError, match="k_new"):
        K.extend_attn(*args(kn_S=4))
    with pytest.raises(_lib.KvqError, match="Hq % Hkv"):
        K.extend_attn(*args(Hq=3, Hkv=2))
    with pytest.raises(_lib.KvqError, match="exceeds"):
        K.extend_attn(*args()[:7], 12, *args()[8:])  # the store holds 11 tokens
    with pytest.raises(_lib.KvqError, match="query dtype"):
        K.extend_attn(*args(q_dtype=torch.bfloat16))
    buf = ctypes.create_string_buffer(256)
    assert _lib.load().kvq_kernel_log(buf, 256) == 0, buf.value  # nothing was launched
