"""Logit soft-capping and attention sinks, host side (CPU): the C ABI declares and exports the four ``_ex`` entry points
with the options record, the Python wrappers take ``softcap`` / ``sinks`` and call ``_ex`` only when one of them is set, the
fused HF forward resolves the modifiers only for a cache built with ``score_modifiers=True`` (keyword over module attribute,
None is off; every other cache still refuses them), sinks are converted once per module, and the prompt forward with a
modifier agrees with transformers' eager attention of Gemma 2 and gpt-oss."""
import ctypes
import inspect
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = ("kvq_decode_attn_ex", "kvq_decode_step_ex", "kvq_decode_step_dev_ex", "kvq_extend_attn_ex")
needs_hf = pytest.mark.skipif("not __import__('efficient_llm_inference_amd.quantization.fused_attention', fromlist=['x']).available()")


def test_header_and_library_have_the_ex_entry_points():
    from efficient_llm_inference_amd import _lib
    header = open(os.path.join(ROOT, "include", "kvq_hip.h")).read()
    assert re.search(r"typedef struct \{\s*int64_t window;[^}]*const int32_t\* kv_start;[^}]*float softcap;[^}]*const float\* sinks;[^}]*\} kvq_attn_opts_t;",
                     header)
    lib = _lib.load()
    for name in EX:
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.EXPORTS
        fn, padded = getattr(lib, name), getattr(lib, name[:-3] + "_padded")
        # the padded argument list with the record in place of (window, kv_start)
        at, pt = list(fn.argtypes), list(padded.argtypes)
        i = at.index(ctypes.POINTER(_lib.KvqAttnOpts))
        assert at[:i] == pt[:i] and at[i + 1:] == pt[i + 2:] and pt[i:i + 2] == [ctypes.c_int64, ctypes.c_void_p]
    assert "kvq_decode_step_layers_ex" not in header.replace("no `_ex` form", "")
    f = dict((n, (t, getattr(_lib.KvqAttnOpts, n).offset)) for n, t in _lib.KvqAttnOpts._fields_)
    assert [f[n][1] for n in ("window", "kv_start", "softcap", "sinks")] == [0, 8, 16, 24] and ctypes.sizeof(_lib.KvqAttnOpts) == 32


def test_null_opts_and_bad_softcap_are_refused_before_the_device():
    from efficient_llm_inference_amd import _lib
    lib = _lib.load()
    for name in EX:
        fn = getattr(lib, name)
        args = [None if t is ctypes.c_void_p or hasattr(t, "contents") else 0 for t in fn.argtypes]
        assert fn(*args) == -1  # KVQ_E_NULL
        assert b"NULL opts" in lib.kvq_last_error_string()


def test_wrappers_take_the_keywords_and_call_ex_only_when_set():
    from efficient_llm_inference_amd import _lib, kernels as K
    from efficient_llm_inference_amd.quantization.ops import QuantizedKVCache
    for fn in (K.decode_attn, K.decode_step, K.decode_step_dev, K.extend_attn, QuantizedKVCache.attend, QuantizedKVCache.extend):
        p = inspect.signature(fn).parameters
        assert p["softcap"].default == 0.0 and p["sinks"].default is None, fn
    lib = types.SimpleNamespace(**{b + s: b + s for b in ("kvq_decode_attn", "kvq_extend_attn") for s in ("", "_window", "_padded", "_ex")})
    ks = ctypes.c_void_p(4096)
    assert K._windowed_entry(lib, "kvq_decode_attn", 0, None) == ("kvq_decode_attn", ())
    assert K._windowed_entry(lib, "kvq_decode_attn", 7, None, 0.0, None) == ("kvq_decode_attn_window", (7,))
    assert K._windowed_entry(lib, "kvq_extend_attn", 7, ks, 0.0, None) == ("kvq_extend_attn_padded", (7, ks))
    for cap, sinks in ((5.0, None), (0.0, ctypes.c_void_p(8192)), (5.0, ctypes.c_void_p(8192))):
        name, (ref,) = K._windowed_entry(lib, "kvq_decode_attn", 7, ks, cap, sinks)
        o = ref._obj
        assert name == "kvq_decode_attn_ex" and isinstance(o, _lib.KvqAttnOpts)
        assert (o.window, o.kv_start, o.softcap, o.sinks) == (7, 4096, cap, None if sinks is None else 8192)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(_lib.KvqError, match="softcap"):
            K._softcap_arg(bad, "decode_attn")
    assert K._softcap_arg(0, "x") == 0.0 and K._softcap_arg(30, "x") == 30.0
    dev = torch.device("cpu")
    assert K._sinks_arg(None, 4, dev, "x") is None
    for bad in (torch.zeros(4, dtype=torch.float16), torch.zeros(5), torch.zeros(8)[::2], [0.0] * 4):
        with pytest.raises(_lib.KvqError, match="sinks"):
            K._sinks_arg(bad, 4, dev, "x")
    t = torch.zeros(4)
    assert K._sinks_arg(t, 4, dev, "x").value == t.data_ptr()


@needs_hf
def test_guard_resolution():
    from efficient_llm_inference_amd.quantization import fused_attention as FA
    mod = types.SimpleNamespace(layer_idx=0, attn_logit_softcapping=50.0)
    assert FA._layer_softcap(mod, {}) == 50.0
    assert FA._layer_softcap(mod, {"softcap": 30.0}) == 30.0  # the keyword wins
    assert FA._layer_softcap(mod, {"softcap": None}) == 50.0  # None: the module's
    assert FA._layer_softcap(types.SimpleNamespace(layer_idx=0), {"softcap": None}) == 0.0  # None is off
    assert FA._layer_softcap(types.SimpleNamespace(layer_idx=0, attn_logit_softcapping=None), {}) == 0.0
    for bad in (0.0, -3.0, float("inf")):
        with pytest.raises(RuntimeError, match="soft cap"):
            FA._layer_softcap(types.SimpleNamespace(layer_idx=0), {"softcap": bad})
    # every owner without score_modifiers = True keeps today's refusals, before any tensor is touched
    plain = types.SimpleNamespace(layer_idx=0)
    owners = [FA.FusedQuantizedCache.__new__(FA.FusedQuantizedCache), types.SimpleNamespace(score_modifiers=False)]
    prev = FA._ACTIVE
    try:
        for owner in owners:
            FA._ACTIVE = owner
            with pytest.raises(RuntimeError, match="softcap"):
                FA._fused_attention_forward(plain, None, None, None, softcap=30.0)
            with pytest.raises(RuntimeError, match="s_aux"):
                FA._fused_attention_forward(plain, None, None, None, s_aux=torch.zeros(4))
            with pytest.raises(RuntimeError, match="sinks"):
                FA._fused_attention_forward(types.SimpleNamespace(layer_idx=0, sinks=1), None, None, None)
            with pytest.raises(RuntimeError, match="attn_logit_softcapping"):
                FA._fused_attention_forward(types.SimpleNamespace(layer_idx=0, attn_logit_softcapping=50.0), None, None, None)
    finally:
        FA._ACTIVE = prev
    assert inspect.signature(FA.FusedQuantizedCache.__init__).parameters["score_modifiers"].default is False
    from efficient_llm_inference_amd.benchmarking import benchmarker
    assert "score_modifiers=self.score_modifiers" in inspect.getsource(benchmarker.KVCacheBenchmarker._generate_fused)


@needs_hf
def test_sinks_are_converted_once_per_module():
    from efficient_llm_inference_amd.quantization import fused_attention as FA
    owner = types.SimpleNamespace(_sinks={})
    param = torch.nn.Parameter(torch.arange(8, dtype=torch.bfloat16))
    m1, m2 = types.SimpleNamespace(layer_idx=0, sinks=param), types.SimpleNamespace(layer_idx=1, sinks=None)
    a = FA._layer_sinks(owner, m1, {"s_aux": param}, 8, "cpu")
    assert a.dtype == torch.float32 and a.shape == (8,) and a.is_contiguous() and torch.equal(a, param.detach().float())
    assert FA._layer_sinks(owner, m1, {"s_aux": param}, 8, "cpu") is a  # the same tensor, hence the same pointer, every step
    assert FA._layer_sinks(owner, m1, {}, 8, "cpu") is a                # module.sinks is the same source
    assert FA._layer_sinks(owner, m2, {}, 8, "cpu") is None and FA._layer_sinks(owner, m2, {"sinks": None}, 8, "cpu") is None
    other = torch.ones(8)
    b = FA._layer_sinks(owner, m2, {"sinks": other}, 8, "cpu")  # the `sinks` keyword; another module, another entry
    assert b is not a and torch.equal(b, other) and len(owner._sinks) == 2
    with torch.no_grad():
        param.add_(1.0)  # an in-place update of the source is seen
    assert torch.equal(FA._layer_sinks(owner, m1, {}, 8, "cpu"), param.detach().float())
    with pytest.raises(RuntimeError, match="one logit per query head"):
        FA._layer_sinks(owner, m1, {"s_aux": torch.zeros(7)}, 8, "cpu")


@needs_hf
@pytest.mark.parametrize("which", ["gemma2", "gpt_oss"])
def test_prompt_forward_with_a_modifier_is_transformers_eager_attention(which):
    """the empty-store branch of the fused forward for an opted-in cache, on the CPU, against the model's own eager function:
    causal, and banded when the prompt is longer than the window"""
    import importlib
    from efficient_llm_inference_amd.quantization import fused_attention as FA
    hf = importlib.import_module(f"transformers.models.{which}.modeling_{which}")
    torch.manual_seed(0)
    B, Hq, Hkv, n, D, W = 2, 8, 2, 24, 16, 9
    q, k, v = torch.randn(B, Hq, n, D), torch.randn(B, Hkv, n, D), torch.randn(B, Hkv, n, D)
    module = types.SimpleNamespace(layer_idx=0, num_key_value_groups=Hq // Hkv, training=False, head_dim=D)
    kw = dict(scaling=0.3)
    if which == "gemma2":
        module.attn_logit_softcapping = 2.0
        kw["softcap"] = 2.0
    else:
        module.sinks = torch.nn.Parameter(torch.randn(Hq))
        kw["s_aux"] = module.sinks
    owner = FA.FusedQuantizedCache.__new__(FA.FusedQuantizedCache)  # no store: the prompt branch never touches one
    owner.score_modifiers, owner._sinks, owner.kv_start, owner.t_dev = True, {}, None, None
    owner.cache = types.SimpleNamespace(layers=[types.SimpleNamespace(past=0)])
    i = torch.arange(n)
    prev = FA._ACTIVE
    FA._ACTIVE = owner
    try:
        for window in (None, W):
            vis = i[None, :] <= i[:, None]
            if window:
                vis = vis & (i[None, :] > i[:, None] - window)
            mask = torch.zeros(n, n).masked_fill(~vis, float("-inf"))[None, None]
            want, _ = hf.eager_attention_forward(module, q, k, v, mask, **kw)
            got, _ = FA._fused_attention_forward(module, q, k, v, None, sliding_window=window, **kw)
            assert got.shape == want.shape == (B, n, Hq, D)
            assert torch.allclose(got, want, rtol=1e-5, atol=1e-6), (which, window, (got - want).abs().max())
            # the left-padded prompt branch takes the model's materialised mask
            owner.kv_start = torch.zeros(B, dtype=torch.int32)
            got, _ = FA._fused_attention_forward(module, q, k, v, mask.expand(B, 1, n, n), sliding_window=window, **kw)
            owner.kv_start = None
            assert torch.allclose(got, want, rtol=1e-5, atol=1e-6), (which, window, "mask")
    finally:
        FA._ACTIVE = prev
