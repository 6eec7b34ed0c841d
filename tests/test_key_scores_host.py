"""CPU-side checks of kvq_key_scores and of the score policy on top of it: the symbols are exported, bad arguments are refused
before anything touches a device, the workspace size is non-decreasing in T, and ``keep_indices_top_scores`` (which runs on
whatever device its scores live on) equals its numpy restatement on crafted scores. No compute calls on a GPU here."""
import ctypes
from ctypes import byref

import numpy as np
import pytest
import torch

from tests.key_score_cases import np_keep_top_scores


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


def refusals(lib):
    """(return code, error string) of kvq_key_scores for every documented refusal; shared with tests/test_gpu_key_scores.py.
    The pointers are never dereferenced: every call fails validation."""
    from efficient_llm_inference_amd import _lib
    fake = ctypes.c_void_p(0x1000)
    st = _lib.KvqStrides(0, 1 << 20, 1 << 16, 128)

    def call(q=fake, k=fake, sc=fake, mass=fake, ws=fake, dims=None, dtype=0, kb=8, qs=(8, 8, 8), ms=(1 << 20, 1 << 16), n_ws=1 << 30):
        d = _dims() if dims is None else dims
        rc = lib.kvq_key_scores(q, *qs, k, byref(st), sc, kb, mass, *ms, 0, dtype, ctypes.c_float(0.1), ws, n_ws,
                                None if d is False else byref(d), None)
        return rc, lib.kvq_last_error_string().decode()

    out = {"NULL dims": call(dims=False), "NULL q": call(q=None), "NULL k_store": call(k=None), "NULL k_scales": call(sc=None),
           "NULL mass": call(mass=None), "NULL workspace": call(ws=None)}
    for name, bad in (("D 32", dict(D=32)), ("D 256", dict(D=256)), ("S > T", dict(S=101)), ("S = 0", dict(S=0)),
                      ("nq = 17", dict(Hq=34, Hkv=2)), ("Hq % Hkv", dict(Hq=6, Hkv=4)), ("T = 0", dict(T=0, S=1)), ("B = 0", dict(B=0))):
        out[name] = call(dims=_dims(**bad))
    out["fp32"] = call(dtype=2)
    out["k_bits 5"] = call(kb=5)
    out["q stride"] = call(qs=(8, 4, 8))
    out["mass stride"] = call(ms=(1 << 20, 50))
    out["small workspace"] = call(n_ws=3)
    return out


def check_refusals(got):
    for name in ("NULL dims", "NULL q", "NULL k_store", "NULL k_scales", "NULL mass", "NULL workspace"):
        assert got[name][0] == -1 and "NULL" in got[name][1], (name, got[name])
    for name, word in (("D 32", "head_dim must be 64 or 128"), ("D 256", "head_dim must be 64 or 128"), ("S > T", "S <= T"),
                       ("S = 0", "must be positive"), ("nq = 17", "Hq / Hkv <= 16"), ("Hq % Hkv", "Hq % Hkv == 0"),
                       ("T = 0", "must be positive"), ("B = 0", "must be positive"), ("k_bits 5", "k_bits must be 8 or 4"),
                       ("q stride", "multiples of 8"), ("mass stride", "mass must be fp32"), ("small workspace", "workspace of 3 floats")):
        assert got[name][0] == -2 and word in got[name][1], (name, got[name])
    assert got["fp32"][0] == -3 and "dtype 2 not supported" in got["fp32"][1], got["fp32"]


def test_symbols_exported(lib):
    from efficient_llm_inference_amd import _lib
    for name in ("kvq_key_scores", "kvq_key_scores_workspace"):
        assert hasattr(lib, name) and name in _lib.EXPORTS


def test_refused_before_any_device_work(lib):
    check_refusals(refusals(lib))
    assert lib.kvq_timing_armed() == 0


def test_workspace_refuses_bad_dims(lib):
    ws = lib.kvq_key_scores_workspace
    assert ws(None) == -1
    for bad in (dict(D=32), dict(D=256), dict(S=0), dict(S=101), dict(T=0, S=1), dict(Hq=6, Hkv=4), dict(Hq=34, Hkv=2), dict(B=0)):
        assert ws(byref(_dims(**bad))) == -1, bad
    assert ws(byref(_dims())) >= 1


def test_workspace_non_decreasing_in_T(lib):
    """A workspace taken at the store's capacity covers every shorter context (what QuantizedKVCache.key_scores does)."""
    for B, Hq, Hkv, S, D in ((1, 32, 8, 64, 128), (8, 32, 8, 1, 128), (3, 16, 16, 17, 64), (1, 8, 1, 1, 64)):
        prev = 0
        for T in list(range(S, 2000, 37)) + [16384, 100000]:
            n = lib.kvq_key_scores_workspace(byref(_dims(B, Hq, Hkv, T, S, D)))
            assert n >= max(prev, 1), (B, Hq, Hkv, S, D, T)
            prev = n


# ---------------------------------------------------------------------------------------------- the policy, on CPU tensors

def crafted_scores(T=97, seed=0):
    """scores with ties (a few distinct values), isolated peaks (what pooling spreads) and a plateau"""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 6, T).astype(np.float32) * 0.25
    s[[10, 40, 41, 77]] = [9.0, 7.0, 7.0, 9.0]
    s[55:60] = 3.0
    return s


POLICY_ARGS = [dict(budget=20), dict(budget=20, pool=3), dict(budget=20, pool=7), dict(budget=30, prefix_len=4, recent=8, pool=3),
               dict(budget=12, prefix_len=4, recent=8), dict(budget=13, prefix_len=4, recent=8, pool=7),
               dict(budget=96, prefix_len=50, recent=46), dict(budget=1), dict(budget=5, recent=5), dict(budget=0)]


def check_policy(device):
    from efficient_llm_inference_amd.cache.implementations import keep_indices_top_scores
    for seed in (0, 1):
        s = crafted_scores(seed=seed)
        for kw in POLICY_ARGS:
            got = keep_indices_top_scores(torch.from_numpy(s).to(device), **kw)
            ref = np_keep_top_scores(s, **kw)
            assert got.dtype == torch.int32 and got.device.type == torch.device(device).type
            assert got.tolist() == ref, (seed, kw)
            assert len(ref) == kw["budget"]
    s = torch.from_numpy(crafted_scores())
    # keep all: the budget covers T, or the protected ranges meet / overlap
    for kw in (dict(budget=97), dict(budget=200), dict(budget=5, prefix_len=50, recent=47), dict(budget=5, prefix_len=90, recent=90)):
        assert keep_indices_top_scores(s.to(device), **kw) is None, kw


def test_policy_equals_numpy_rule():
    check_policy("cpu")


def test_policy_refusals():
    from efficient_llm_inference_amd.cache.implementations import keep_indices_top_scores
    s = torch.from_numpy(crafted_scores())
    with pytest.raises(ValueError, match="smaller than the protected"):
        keep_indices_top_scores(s, 11, prefix_len=4, recent=8)
    with pytest.raises(ValueError, match="pool must be odd"):
        keep_indices_top_scores(s, 20, pool=4)
    with pytest.raises(ValueError, match="pool must be odd"):
        keep_indices_top_scores(s, 20, pool=0)
    with pytest.raises(ValueError, match="1-D"):
        keep_indices_top_scores(s[None], 20)
    with pytest.raises(ValueError, match=">= 0"):
        keep_indices_top_scores(s, -1)
    with pytest.raises(TypeError):
        keep_indices_top_scores(s, 2.5)


def test_top_scores_is_not_a_trim_policy():
    """its signature differs (scores, not T): QuantizedKVCache.trim keeps the positional policies only"""
    from efficient_llm_inference_amd.cache.implementations import KEEP_INDEX_FNS
    assert "top_scores" not in KEEP_INDEX_FNS and len(KEEP_INDEX_FNS) == 5
