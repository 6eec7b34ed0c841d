"""CPU-side checks of the multi-token attention entry points (kvq_extend_attn): exported, and bad arguments are
refused before anything touches a device. Plus the float64 causal oracle of tests/test_gpu_extend_attn.py at S = 1
against the decode oracle. No compute calls on a GPU here."""
import ctypes
from ctypes import byref

import numpy as np
import pytest

from oracle import kvq_oracle as O


@pytest.fixture(scope="module")
def lib():
    import os

    from efficient_llm_inference_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _dims(B=1, Hq=8, Hkv=2, T=100, S=4, D=128):
    from efficient_llm_inference_amd import _lib
    return _lib.KvqExtendDims(B, Hq, Hkv, T, S, D)


def test_extend_symbols_exported(lib):
    from efficient_llm_inference_amd import _lib
    for name in ("kvq_extend_attn", "kvq_extend_attn_workspace"):
        assert hasattr(lib, name) and name in _lib.EXPORTS


def test_extend_workspace_refuses_bad_dims(lib):
    ws = lib.kvq_extend_attn_workspace
    assert ws(None) == -1
    for bad in (dict(D=32), dict(D=256), dict(D=80), dict(D=96), dict(S=0), dict(T=-1), dict(Hq=6, Hkv=4),
                dict(Hq=34, Hkv=2), dict(B=0), dict(Hkv=0)):
        assert ws(byref(_dims(**bad))) == -1, bad
    assert ws(byref(_dims())) >= 0
    assert ws(byref(_dims(T=0))) == 0  # no stored tokens: one split, no partials


def test_extend_workspace_non_decreasing_in_T(lib):
    """A workspace taken at the store's capacity covers every shorter context (what QuantizedKVCache.extend does)."""
    for B, Hq, Hkv, S, D in ((1, 32, 8, 512, 128), (8, 32, 8, 4, 128), (3, 16, 16, 17, 64), (1, 8, 1, 1, 64)):
        prev = 0
        for T in list(range(0, 2000, 37)) + [16384, 100000]:
            n = lib.kvq_extend_attn_workspace(byref(_dims(B, Hq, Hkv, T, S, D)))
            assert n >= prev, (B, Hq, Hkv, S, D, T)
            prev = n


def test_extend_attn_refuses_before_any_device_work(lib):
    from efficient_llm_inference_amd import _lib
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: every call below fails validation
    st = _lib.KvqStrides(0, 0, 0, 0)

    def call(q=fake, kn=fake, vn=fake, out=fake, dims=None, dtype=0, kb=8, vb=8, strides=(8, 8, 8)):
        d = _dims() if dims is None else dims
        return lib.kvq_extend_attn(q, *strides, fake, byref(st), fake, kb, fake, byref(st), fake, vb,
                                   kn, *strides, vn, *strides, out, *strides, dtype, ctypes.c_float(0.1),
                                   fake, 1 << 20, None if d is False else byref(d), None)

    assert call(dims=False) == -1 and b"NULL" in lib.kvq_last_error_string()
    assert call(q=None) == -1
    assert call(kn=None) == -1
    assert call(out=None) == -1
    for bad in (dict(D=32), dict(D=256), dict(S=0), dict(Hq=6, Hkv=4), dict(T=-5)):
        assert call(dims=_dims(**bad)) == -2, bad
        assert b"bad dims" in lib.kvq_last_error_string()
    assert call(dtype=2) == -3  # fp32 tensors are not a compute dtype here
    assert call(kb=5) == -2
    assert lib.kvq_timing_armed() == 0


def test_causal_oracle_at_one_token_equals_decode_oracle():
    rng = np.random.default_rng(2)
    B, Hq, Hkv, T, D = 2, 8, 2, 50, 64
    kv = rng.standard_normal((2, 1, B, Hkv, T, D)).astype(np.float16)
    kq, _, ks = O.quantize_tokens(kv[0], "int8")
    vq, _, vs = O.quantize_tokens(kv[1], "int4")
    q = rng.standard_normal((B, Hq, D)).astype(np.float32)
    kn = rng.standard_normal((B, Hkv, D)).astype(np.float32)
    vn = rng.standard_normal((B, Hkv, D)).astype(np.float32)
    a = O.extend_attention(q[:, :, None], kq[0], ks[0], "int8", vq[0], vs[0], "int4", D, 0.125, kn[:, :, None], vn[:, :, None])
    b = O.decode_attention(q, kq[0], ks[0], "int8", vq[0], vs[0], "int4", D, 0.125, kn, vn)
    np.testing.assert_allclose(a[:, :, 0], b, rtol=1e-12, atol=1e-12)
    # the causal mask: the first row of a chunk sees the past and chunk token 0 only
    S = 3
    qs = rng.standard_normal((B, Hq, S, D)).astype(np.float32)
    kns = rng.standard_normal((B, Hkv, S, D)).astype(np.float32)
    vns = rng.standard_normal((B, Hkv, S, D)).astype(np.float32)
    c = O.extend_attention(qs, kq[0], ks[0], "int8", vq[0], vs[0], "int4", D, 0.125, kns, vns)
    d = O.decode_attention(qs[:, :, 0], kq[0], ks[0], "int8", vq[0], vs[0], "int4", D, 0.125, kns[:, :, 0], vns[:, :, 0])
    np.testing.assert_allclose(c[:, :, 0], d, rtol=1e-12, atol=1e-12)
