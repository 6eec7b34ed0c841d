"""Sliding-window attention over the quantised store, host side (CPU): the C ABI declares and exports the four windowed
entry points, the fused HF forward resolves each layer's window (and still refuses soft-capping and sinks), the mask
function leaves a local window to the kernels, the Python validators reject negative windows, and the float64
model the GPU tests compare against (tests/attn_ref.py) agrees under a window with a brute-force masked softmax."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from tests.conftest import ROOT
from tests.attn_ref import attention, decode_lo

WINDOW_SYMBOLS = ("kvq_decode_attn_window", "kvq_decode_step_window", "kvq_decode_step_dev_window", "kvq_extend_attn_window")


def test_header_declares_and_library_exports_the_window_entry_points():
    hdr = open(os.path.join(ROOT, "include", "kvq_hip.h")).read()
    for name in WINDOW_SYMBOLS:
        m = re.search(r"int " + name + r"\(([^;]*)\);", hdr)
        assert m, name
        # `int64_t window` directly after `float sm_scale`
        assert re.search(r"float sm_scale,\s*int64_t window,", m.group(1)), name
    from efficient_llm_inference_amd import _lib
    lib = _lib.load()
    for name in WINDOW_SYMBOLS:
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr), name


def test_layer_window_resolution():
    from efficient_llm_inference_amd.quantization import fused_attention as FA
    # the keyword wins over the attribute; None means full attention
    assert FA._layer_window(types.SimpleNamespace(sliding_window=16), {"sliding_window": 64}) == 64
    assert FA._layer_window(types.SimpleNamespace(sliding_window=16), {}) == 16
    assert FA._layer_window(types.SimpleNamespace(sliding_window=16), {"sliding_window": None}) == 16
    assert FA._layer_window(types.SimpleNamespace(), {"sliding_window": None}) == 0
    assert FA._layer_window(types.SimpleNamespace(sliding_window=None), {}) == 0
    with pytest.raises(RuntimeError):
        FA._layer_window(types.SimpleNamespace(), {"sliding_window": -3})


@pytest.mark.skipif("not __import__('efficient_llm_inference_amd.quantization.fused_attention', fromlist=['x']).available()")
def test_window_is_implemented_softcap_and_sinks_still_refused():
    from efficient_llm_inference_amd.quantization import fused_attention as FA
    plain = types.SimpleNamespace(layer_idx=0)
    impl = ("sliding_window",)
    FA._reject_unsupported_variants(plain, {"sliding_window": 4096}, implemented=impl)
    FA._reject_unsupported_variants(types.SimpleNamespace(layer_idx=0, sliding_window=7), {}, implemented=impl)
    for kw in ({"softcap": 50.0}, {"s_aux": object()}, {"sinks": object()}):
        with pytest.raises(RuntimeError, match=next(iter(kw))):
            FA._reject_unsupported_variants(plain, {"sliding_window": 64, **kw}, implemented=impl)
    for attr in ("sinks", "attn_logit_softcapping"):
        with pytest.raises(RuntimeError, match=attr):
            FA._reject_unsupported_variants(types.SimpleNamespace(layer_idx=0, sliding_window=64, **{attr: 7}), {},
                                            implemented=impl)
    # through the forward with a FusedQuantizedCache owner: the window passes the guard, soft-capping does not (the guard
    # runs before any tensor is touched)
    prev = FA._ACTIVE
    FA._ACTIVE = FA.FusedQuantizedCache.__new__(FA.FusedQuantizedCache)
    try:
        with pytest.raises(RuntimeError, match="softcap"):
            FA._fused_attention_forward(plain, None, None, None, sliding_window=128, softcap=30.0)
        with pytest.raises(RuntimeError, match="sinks"):
            FA._fused_attention_forward(types.SimpleNamespace(layer_idx=0, sinks=1), None, None, None, sliding_window=128)
    finally:
        FA._ACTIVE = prev


@pytest.mark.skipif("not __import__('efficient_llm_inference_amd.quantization.fused_attention', fromlist=['x']).available()")
def test_fused_mask_leaves_a_local_window_to_the_kernels():
    from transformers.masking_utils import sdpa_mask

    from efficient_llm_inference_amd.quantization import fused_attention as FA
    # no padding: None, for decode and for a multi-token forward, with or without a past
    for q_len, kv_len in ((1, 100), (16, 116), (100, 100)):
        assert FA._fused_mask(1, q_len, kv_len, 0, 0, attention_mask=torch.ones(1, kv_len, dtype=torch.bool),
                              local_size=64) is None
        assert FA._fused_mask(1, q_len, kv_len, 0, 0, attention_mask=None, local_size=64) is None
    # a real padding mask: exactly sdpa_mask
    pad = torch.ones(2, 40, dtype=torch.bool)
    pad[0, :5] = False
    got = FA._fused_mask(2, 8, 40, 0, 0, attention_mask=pad, local_size=16)
    want = sdpa_mask(2, 8, 40, 0, 0, attention_mask=pad, local_size=16)
    assert got is not None and torch.equal(got, want)


def test_validators_reject_negative_windows():
    from efficient_llm_inference_amd import _lib, kernels
    for w in (-1, -4096, 1.5, True):
        with pytest.raises(_lib.KvqError, match="window"):
            kernels._window_arg(w, "decode_attn")
    assert kernels._window_arg(0, "x") == 0 and kernels._window_arg(64, "x") == 64
    # the public wrappers check the window before anything else (no GPU needed to get the error)
    with pytest.raises(_lib.KvqError, match="window"):
        kernels.decode_attn(None, None, None, "int8", None, None, "int8", 0, None, None, 1.0, window=-1)
    with pytest.raises(_lib.KvqError, match="window"):
        kernels.extend_attn(None, None, None, "int8", None, None, "int8", 0, None, None, None, None, 1.0, window=-2)
    with pytest.raises(_lib.KvqError, match="window"):
        kernels.decode_step(None, None, None, None, 0, None, None, 1.0, window=-1)
    with pytest.raises(_lib.KvqError, match="window"):
        kernels.decode_step_dev(None, None, None, None, None, 1, None, None, 1.0, window=-1)
    from efficient_llm_inference_amd import QuantizedKVCache
    qc = QuantizedKVCache(1, "int8", device="cpu")
    with pytest.raises(_lib.KvqError, match="window"):
        qc.attend(0, torch.zeros(1, 1, 64), window=-5)
    with pytest.raises(_lib.KvqError, match="window"):
        qc.extend(0, torch.zeros(1, 1, 2, 64), torch.zeros(1, 1, 2, 64), torch.zeros(1, 1, 2, 64), window=-5)


def test_the_library_rejects_negative_windows():
    from efficient_llm_inference_amd import _lib
    lib = _lib.load()
    d = _lib.KvqAttnDims(1, 1, 1, 4, 64)
    rc = lib.kvq_decode_attn_window(None, 0, 0, None, None, None, 8, None, None, None, 8, None, 0, 0, None, 0, 0,
                                    None, 0, 0, 0, ctypes.c_float(1.0), -1, None, 0, ctypes.byref(d), None)
    assert rc != 0 and "window" in lib.kvq_last_error_string().decode()


@pytest.mark.parametrize("T,S,W", [(0, 9, 3), (20, 1, 1), (20, 1, 5), (20, 7, 4), (5, 30, 8), (12, 6, 0), (12, 6, 40)])
def test_windowed_reference_equals_brute_force(T, S, W):
    rng = np.random.default_rng(T * 100 + S * 10 + W)
    B, Hq, Hkv, D = 2, 4, 2, 16
    q = rng.standard_normal((B, Hq, S, D))
    kd = rng.standard_normal((B, Hkv, T + S, D))
    vd = rng.standard_normal((B, Hkv, T + S, D))
    got = attention(q, kd, vd, T + np.arange(S), 0.3, W)
    for b in range(B):
        for h in range(Hq):
            for s in range(S):
                p = T + s
                lo = max(0, p - W + 1) if W else 0
                keys = np.arange(lo, p + 1)
                sc = kd[b, h // 2, keys] @ q[b, h, s] * 0.3
                e = np.exp(sc - sc.max())
                want = (e / e.sum()) @ vd[b, h // 2, keys]
                np.testing.assert_allclose(got[b, h, s], want, rtol=1e-12, atol=1e-12)
    # decode's first stored row: with the new token at T, without it the last stored token is the query's own
    assert decode_lo(100, 64) == 37 and decode_lo(100, 64, has_new=False) == 36
    assert decode_lo(10, 64) == 0 and decode_lo(10, 0) == 0 and decode_lo(10, 1) == 10
