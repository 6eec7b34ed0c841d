"""Left-padded batches (per-row key starts) in attention over the quantised store, host side (CPU): the C ABI declares and
exports the four padded entry points, the Python validators refuse a bad ``kv_start`` before any launch, the float64 model the
GPU tests compare against (tests/attn_ref.py) agrees with a brute-force masked softmax (rows without a visible key are zeros in both), and
``FusedQuantizedCache.set_left_padding`` accepts left padding only while a cache without it refuses masks as before."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from tests.conftest import ROOT
from tests.attn_ref import attention

PADDED_SYMBOLS = ("kvq_decode_attn_padded", "kvq_decode_step_padded", "kvq_decode_step_dev_padded", "kvq_extend_attn_padded")


def test_header_declares_and_library_exports_the_padded_entry_points():
    hdr = open(os.path.join(ROOT, "include", "kvq_hip.h")).read()
    for name in PADDED_SYMBOLS:
        m = re.search(r"int " + name + r"\(([^;]*)\);", hdr)
        assert m, name
        # `const int32_t* kv_start` directly after `int64_t window`, itself directly after `float sm_scale`
        assert re.search(r"float sm_scale,\s*int64_t window,\s*const int32_t\* kv_start,", m.group(1)), name
        # otherwise the `_window` signature
        w = re.search(r"int " + name.replace("_padded", "_window") + r"\(([^;]*)\);", hdr).group(1)
        norm = lambda t: re.sub(r"\s+", " ", t)
        assert norm(m.group(1)).replace(" const int32_t* kv_start,", "") == norm(w), name
    from efficient_llm_inference_amd import _lib
    lib = _lib.load()
    for name in PADDED_SYMBOLS:
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr) and name in _lib.EXPORTS, name


def test_validators_refuse_a_bad_kv_start_before_any_launch():
    from efficient_llm_inference_amd import _lib, kernels
    dev = torch.device("cpu")
    ok = torch.zeros(3, dtype=torch.int32)
    assert kernels._kv_start_arg(None, 3, dev, "x") is None
    assert kernels._kv_start_arg(ok, 3, dev, "x") is not None
    for bad, why in ((torch.zeros(3, dtype=torch.int64), "int32"), (torch.zeros(3), "int32"), (torch.zeros(4, dtype=torch.int32), "B"),
                     (torch.zeros(3, 1, dtype=torch.int32), "B"), (torch.zeros(6, dtype=torch.int32)[::2], "contiguous"),
                     ([0, 0, 0], "tensor")):
        with pytest.raises(_lib.KvqError, match=why):
            kernels._kv_start_arg(bad, 3, dev, "decode_attn")
    with pytest.raises(_lib.KvqError, match="lives on"):  # the wrong device
        kernels._kv_start_arg(ok, 3, torch.device("meta"), "decode_attn")
    # through the public wrappers: refused on the host (these CPU tensors never reach a launch)
    q = torch.zeros(3, 4, 64, dtype=torch.float16)
    with pytest.raises(_lib.KvqError):
        kernels.decode_attn(q, None, None, "int8", None, None, "int8", 0, q, None, 1.0, kv_start=torch.zeros(3, dtype=torch.int64))
    # a negative window is still refused first
    with pytest.raises(_lib.KvqError, match="window"):
        kernels.decode_attn(None, None, None, "int8", None, None, "int8", 0, None, None, 1.0, window=-1, kv_start=ok)
    with pytest.raises(_lib.KvqError, match="window"):
        kernels.extend_attn(None, None, None, "int8", None, None, "int8", 0, None, None, None, None, 1.0, window=-2, kv_start=ok)
    with pytest.raises(_lib.KvqError, match="window"):
        kernels.decode_step(None, None, None, None, 0, None, None, 1.0, window=-1, kv_start=ok)
    with pytest.raises(_lib.KvqError, match="window"):
        kernels.decode_step_dev(None, None, None, None, None, 1, None, None, 1.0, window=-1, kv_start=ok)


def test_the_library_rejects_negative_windows_in_the_padded_calls():
    """A negative window is KVQ_E_DIMS (-2) in all four padded entry points, as in the windowed ones; the dummy host
    pointers are never dereferenced (the check precedes every launch)."""
    from efficient_llm_inference_amd import _lib
    lib = _lib.load()
    KVQ_E_DIMS = -2
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    st = _lib.KvqStrides(0, 0, 0, 0)
    sp = ctypes.byref(st)
    d = _lib.KvqAttnDims(1, 1, 1, 4, 64)
    e = _lib.KvqExtendDims(1, 1, 1, 4, 2, 64)
    one = ctypes.c_float(1.0)
    eps = ctypes.c_float(1e-8)
    calls = {
        "kvq_decode_attn_padded": lambda w: lib.kvq_decode_attn_padded(p, 0, 0, p, sp, p, 8, p, sp, p, 8, p, 0, 0, p, 0, 0, p, 0, 0, 0,
                                                                     one, w, p, p, 64, ctypes.byref(d), None),
        "kvq_decode_step_padded": lambda w: lib.kvq_decode_step_padded(p, 0, 0, p, 0, 0, p, 0, 0, p, sp, p, 8, p, sp, p, 8, p, 0, 0, 0,
                                                                     one, w, p, eps, p, 64, ctypes.byref(d), None),
        "kvq_decode_step_dev_padded": lambda w: lib.kvq_decode_step_dev_padded(p, 0, 0, p, 0, 0, p, 0, 0, p, sp, p, 8, p, sp, p, 8, p, 0,
                                                                             0, 0, one, w, p, eps, p, 64, ctypes.byref(d), p, None),
        "kvq_extend_attn_padded": lambda w: lib.kvq_extend_attn_padded(p, 0, 0, 0, p, sp, p, 8, p, sp, p, 8, p, 0, 0, 0, p, 0, 0, 0,
                                                                     p, 0, 0, 0, 0, one, w, p, p, 64, ctypes.byref(e), None),
    }
    for name, call in calls.items():
        for w in (-1, -4096):
            assert call(w) == KVQ_E_DIMS, name
            assert "window" in lib.kvq_last_error_string().decode(), name


@pytest.mark.parametrize("T", [0, 1, 64, 65, 200])
@pytest.mark.parametrize("S", [1, 5, 70])
def test_padded_reference_equals_brute_force(T, S):
    rng = np.random.default_rng(T * 100 + S)
    B, Hq, Hkv, D = 5, 4, 2, 8
    q = rng.standard_normal((B, Hq, S, D))
    kd = rng.standard_normal((B, Hkv, T + S, D))
    vd = rng.standard_normal((B, Hkv, T + S, D))
    mid = min(T + S - 1, 70) if T + S > 70 else (T + S) // 2  # mid-tile
    starts = [0, mid, max(T - 1, 0), T, T + S - 1]
    for W in sorted({0, 1, 16, T + S}):
        got = attention(q, kd, vd, T + np.arange(S), 0.3, W, starts)
        zero_rows = 0
        for b in range(B):
            for h in range(Hq):
                for s in range(S):
                    p = T + s
                    lo = max(starts[b], p - W + 1 if W > 0 else 0)
                    keys = [k for k in range(T + S) if lo <= k <= p]
                    if not keys:
                        assert (got[b, h, s] == 0).all()
                        zero_rows += 1
                        continue
                    sc = np.array([kd[b, h // 2, k] @ q[b, h, s] * 0.3 for k in keys])
                    e = np.exp(sc - sc.max())
                    want = sum(w * vd[b, h // 2, k] for w, k in zip(e / e.sum(), keys))
                    np.testing.assert_allclose(got[b, h, s], want, rtol=1e-12, atol=1e-12)
        if S > 1:  # the start T + S - 1 hides every key from the rows before the last
            assert zero_rows > 0


FA_OK = "not __import__('efficient_llm_inference_amd.quantization.fused_attention', fromlist=['x']).available()"


def _bare_cache():
    from efficient_llm_inference_amd.quantization import fused_attention as FA
    fc = FA.FusedQuantizedCache.__new__(FA.FusedQuantizedCache)
    fc.qcache = types.SimpleNamespace(_k=types.SimpleNamespace(device="cpu"))
    fc.kv_start = None
    return fc


@pytest.mark.skipif(FA_OK)
def test_set_left_padding_accepts_left_padding_only():
    fc = _bare_cache()
    m = torch.tensor([[1, 1, 1, 1, 1], [0, 0, 1, 1, 1], [0, 0, 0, 0, 1]])
    ks = fc.set_left_padding(m)
    assert ks.dtype == torch.int32 and ks.tolist() == [0, 2, 4] and fc.kv_start is ks and ks.is_contiguous()
    assert fc.set_left_padding(m.bool()).tolist() == [0, 2, 4]
    for bad in (torch.tensor([[1, 1, 0], [1, 1, 1]]),      # right padding
                torch.tensor([[0, 1, 0, 1], [1, 1, 1, 1]]),  # a hole
                torch.tensor([[0, 0, 0], [0, 1, 1]]),      # an all-padding row
                torch.ones(3), torch.ones(2, 3, 4)):
        with pytest.raises(RuntimeError):
            _bare_cache().set_left_padding(bad)


@pytest.mark.skipif(FA_OK)
def test_a_cache_without_left_padding_still_refuses_masks():
    """The three refusals keep today's text on a cache that never called set_left_padding."""
    from efficient_llm_inference_amd.quantization import fused_attention as FA
    mask = torch.ones(1, 1, 1, 1, dtype=torch.bool)
    mod = types.SimpleNamespace(layer_idx=0)
    prev = FA._ACTIVE
    try:
        for n, past, msg in ((4, 0, "kvq: fused attention does not take a padding mask"),
                             (4, 9, "kvq: fused multi-token attention does not take a padding mask"),
                             (1, 9, "kvq: fused decode attention does not take a padding mask")):
            fc = _bare_cache()
            fc.t_dev, fc.ignore_decode_mask = None, False
            fc.cache = types.SimpleNamespace(layers=[types.SimpleNamespace(past=past)])
            FA._ACTIVE = fc
            q = torch.zeros(1, 2, n, 64, dtype=torch.float16)
            with pytest.raises(RuntimeError) as ei:
                FA._fused_attention_forward(mod, q, q[:, :1], q[:, :1], attention_mask=mask)
            assert str(ei.value) == msg
    finally:
        FA._ACTIVE = prev


@pytest.mark.skipif(FA_OK)
def test_a_left_padded_cache_refuses_eviction_and_key_scores():
    """``kv_start`` holds positions of the un-evicted store and is kept for the life of the cache, and kvq_key_scores has no
    per-row start: on a cache that called set_left_padding every eviction and key_scores raise before anything else is looked
    at (the store is empty and lives on the CPU: no launch), as for a captured decode graph."""
    import weakref
    from efficient_llm_inference_amd.quantization.ops import QuantizedKVCache
    fc = _bare_cache()
    fc.t_dev = None
    qc = fc.qcache = QuantizedKVCache(2, "int8", device="cpu")
    qc._fused_owner = weakref.ref(fc)
    q = torch.zeros(2, 4, 3, 64, dtype=torch.float16)
    calls = {
        "keep_tokens": lambda: qc.keep_tokens([0]),
        "trim": lambda: qc.trim("sliding_window", 4),
        "chunk_summarize": lambda: qc.chunk_summarize(4, 2),
        "evict_by_scores": lambda: qc.evict_by_scores(torch.ones(3), 2),
        "compress_prompt": lambda: qc.compress_prompt([q, q], 2),
        "key_scores": lambda: qc.key_scores(0, q),
    }
    for name, call in calls.items():  # without left padding: the empty-cache refusal, as before
        with pytest.raises(ValueError, match="Empty cache"):
            call()
    fc.set_left_padding(torch.tensor([[1, 1, 1], [0, 1, 1]]))
    for name, call in calls.items():
        with pytest.raises(RuntimeError, match="left-padded") as ei:
            call()
        assert ("un-evicted store" if name != "key_scores" else "no per-row key start") in str(ei.value), (name, str(ei.value))
    fc.t_dev = torch.zeros(1, dtype=torch.int32)  # the captured-graph refusal still comes first
    with pytest.raises(RuntimeError, match="captured decode graph"):
        qc.trim("sliding_window", 4)
