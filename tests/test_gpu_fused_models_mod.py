"""Gemma 2 (logit soft-capping) and gpt-oss (per-head attention sinks) on the fused path: tiny random-init models of both
classes, a sliding and a full layer each (window 16), decode over the quantised store with
``FusedQuantizedCache(score_modifiers=True)`` against the same model on the staged path (HF's eager attention over the
dequantised past), teacher-forced over a 24-token prompt and 8 generated tokens, with the tolerance
tests/test_gpu_benchmarker.py uses for fused against staged. The query / key projections are scaled up so that scores
reach the cap (5.0), the sinks are drawn wide enough to hold real mass: without the modifiers the logits do not agree.
Both models run in fp16, as the fused-against-staged tests of tests/test_gpu_benchmarker.py do (measured on the MI355X with
these weights: worst relative logit error 0.017 for both models in fp16; in bf16 0.040 for Gemma 2 and 0.060 for gpt-oss,
0.014 / 0.015 with the projections left at their initial scale: the staged side's eager attention then rounds scores of
several units to bf16, whatever the modifier).
Also: one multi-token forward into the non-empty cache, one graph-mode decode, and the refusal of both models by a cache
built without the opt-in."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N_PROMPT, N_NEW, N_TURN, WINDOW = 24, 8, 6, 16
TOL = 2e-2  # tests/test_gpu_benchmarker.py: worst |fused - staged| / max |staged| per step


def build(which, head_dim=64, dtype=None):
    """(model on the GPU, tokenizer): 2 layers (sliding, full), hidden 64, fp16 unless told"""
    from efficient_llm_inference_amd.benchmarking.offline import RepeatTokenizer
    torch.manual_seed(7)
    common = dict(vocab_size=128, hidden_size=64, num_hidden_layers=2, head_dim=head_dim, sliding_window=WINDOW,
                  layer_types=["sliding_attention", "full_attention"], max_position_embeddings=256, bos_token_id=0, eos_token_id=127,
                  pad_token_id=None, tie_word_embeddings=False, attn_implementation="eager")
    if which == "gemma2":
        from transformers import Gemma2Config, Gemma2ForCausalLM
        heads = (4, 2) if head_dim == 64 else (2, 1)
        cfg = Gemma2Config(intermediate_size=128, num_attention_heads=heads[0], num_key_value_heads=heads[1],
                           attn_logit_softcapping=5.0, query_pre_attn_scalar=head_dim, **common)
        model, dtype = Gemma2ForCausalLM(cfg), dtype or torch.float16
    else:
        from transformers import GptOssConfig, GptOssForCausalLM
        cfg = GptOssConfig(intermediate_size=64, num_attention_heads=8, num_key_value_heads=1, num_local_experts=2,
                           num_experts_per_tok=2, experts_implementation="batched_mm",  # no host synchronisation: capturable
                           **common)
        model, dtype = GptOssForCausalLM(cfg), dtype or torch.float16
    with torch.no_grad():
        for layer in model.model.layers:
            att = layer.self_attn
            att.q_proj.weight.normal_(0.0, 0.3)  # scores of several units: past the cap of 5 for Gemma 2
            att.k_proj.weight.normal_(0.0, 0.3)
            if getattr(att, "sinks", None) is not None:
                att.sinks.normal_(0.0, 3.0)
    return model.to(device="cuda", dtype=dtype).eval(), RepeatTokenizer(vocab_size=128)


def staged_run(model, ids, turn, dtype):
    """teacher-forcing reference: the tuple path (every token kept, HF's mask applies the window)"""
    import efficient_llm_inference_amd as E
    from efficient_llm_inference_amd.benchmarking import from_legacy_tuple, to_legacy_tuple
    from transformers.cache_utils import DynamicCache
    out = model(input_ids=ids, use_cache=True, past_key_values=DynamicCache())
    logits = out.logits[:, -1, :]
    kv = to_legacy_tuple(out.past_key_values)
    qc = E.QuantizedKVCache(len(kv), "mixed", incremental=False, compute_dtype=dtype)
    qc.init_from_prompt_past(kv)
    first, ref, toks = logits.float(), [], []
    for _ in range(N_NEW):
        nxt = torch.argmax(logits, dim=-1, keepdim=True)
        toks.append(nxt)
        out = model(input_ids=nxt, use_cache=True, past_key_values=from_legacy_tuple(qc.to_past_key_values()))
        logits = out.logits[:, -1, :]
        qc.append_from_past(to_legacy_tuple(out.past_key_values))
        ref.append(logits.float())
    ref_turn = None
    if turn is not None:
        ref_turn = model(input_ids=turn, use_cache=True, past_key_values=from_legacy_tuple(qc.to_past_key_values())).logits.float()
    return first, ref, toks, ref_turn, len(kv)


def rel(got, ref):
    return float((got - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("which,head_dim", [("gemma2", 64), ("gemma2", 256), ("gpt_oss", 64)])
def test_fused_decode_tracks_the_staged_path(which, head_dim):
    from efficient_llm_inference_amd import _lib
    from efficient_llm_inference_amd.quantization import fused_attention as FA
    model, tok = build(which, head_dim)
    with torch.no_grad():
        ids = tok(f"<{N_PROMPT}>", return_tensors="pt").input_ids.cuda()
        turn = tok(f"<{N_TURN}>", return_tensors="pt").input_ids.cuda() if head_dim == 64 else None
        dtype = next(model.parameters()).dtype
        first, ref, toks, ref_turn, n_layers = staged_run(model, ids, turn, dtype)

        # a cache without the opt-in still refuses the model, with today's message
        fc0 = FA.FusedQuantizedCache(n_layers, mode="mixed", compute_dtype=dtype)
        with FA.fused_attention(model, fc0) as cache:
            with pytest.raises(RuntimeError, match="softcap" if which == "gemma2" else "s_aux"):
                model(input_ids=ids, use_cache=True, past_key_values=cache)

        fc = FA.FusedQuantizedCache(n_layers, mode="mixed", compute_dtype=dtype, reserve=N_PROMPT + N_NEW + N_TURN,
                                    score_modifiers=True)
        with FA.fused_attention(model, fc) as cache:
            out = model(input_ids=ids, use_cache=True, past_key_values=cache)
            assert rel(out.logits[:, -1, :].float(), first) < TOL  # the eager prompt forward with the modifier
            _lib.kernel_log_clear()
            worst = 0.0
            for step, nxt in enumerate(toks):
                got = model(input_ids=nxt, use_cache=True, past_key_values=cache).logits[:, -1, :].float()
                worst = max(worst, rel(got, ref[step]))
            log = _lib.kernel_log()
            print(which, head_dim, "worst fused vs staged", worst)
            assert worst < TOL, worst
            merges = [k for k in log if "merge" in k]
            assert merges and all("_mod_k" in k for k in merges), log
            partial_mod = any("_mod_k" in k for k in log if "merge" not in k and k.startswith("decode_attn"))
            assert partial_mod == (which == "gemma2"), log  # a soft cap takes the capped partials, sinks alone the tuned ones
            if turn is not None:  # several tokens into the non-empty cache: kvq_extend_attn_ex
                _lib.kernel_log_clear()
                got = model(input_ids=turn, use_cache=True, past_key_values=cache).logits.float()
                assert any(k.startswith("extend_attn_mod_k<") for k in _lib.kernel_log()), _lib.kernel_log()
                assert rel(got, ref_turn) < TOL, rel(got, ref_turn)
        if which == "gpt_oss":  # converted once per module: one fp32 [Hq] tensor per layer
            assert len(fc._sinks) == n_layers and all(v[2].dtype == torch.float32 for v in fc._sinks.values())

        # the modifiers matter on these weights: the same fused run with them switched off in the model does not agree
        att = [layer.self_attn for layer in model.model.layers]
        saved = [(a.attn_logit_softcapping if which == "gemma2" else a.sinks.detach().clone()) for a in att]
        for a in att:
            if which == "gemma2":
                a.attn_logit_softcapping = None
            else:
                a.sinks.fill_(-6e4)  # no mass (the most negative round value fp16 holds)
        fc2 = FA.FusedQuantizedCache(n_layers, mode="mixed", compute_dtype=dtype, reserve=N_PROMPT + N_NEW, score_modifiers=True)
        with FA.fused_attention(model, fc2) as cache:
            model(input_ids=ids, use_cache=True, past_key_values=cache)
            off = max(rel(model(input_ids=nxt, use_cache=True, past_key_values=cache).logits[:, -1, :].float(), ref[s])
                      for s, nxt in enumerate(toks))
        for a, s in zip(att, saved):
            if which == "gemma2":
                a.attn_logit_softcapping = s
            else:
                a.sinks.copy_(s)
        assert off > 2 * TOL, off


@pytest.mark.parametrize("which", ["gemma2", "gpt_oss"])
def test_graph_decode_with_score_modifiers(which):
    """KVCacheBenchmarker's opt-in: the eager fused decode and the captured one (kvq_decode_step_dev_ex replayed with the same
    sinks pointer) emit the same tokens; without the opt-in the model is refused"""
    from efficient_llm_inference_amd import KVCacheBenchmarker
    model, tok = build(which, dtype=torch.float16)
    bench = KVCacheBenchmarker(model, tok, device="cuda")
    bench.fused_attention = True
    with pytest.raises(RuntimeError, match="softcap" if which == "gemma2" else "s_aux"):
        bench.generate_with_quantized_kv(f"<{N_PROMPT}>", N_NEW, mode="mixed")
    bench.score_modifiers = True
    eager = bench.generate_with_quantized_kv(f"<{N_PROMPT}>", N_NEW, mode="mixed")
    bench.graph_decode = True
    graphed = bench.generate_with_quantized_kv(f"<{N_PROMPT}>", N_NEW, mode="mixed")
    assert graphed[1] == eager[1] == N_NEW and graphed[0] == eager[0] and graphed[2] == eager[2]
