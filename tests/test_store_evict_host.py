"""Host side of eviction inside the quantised store (no GPU): the index functions QuantizedKVCache.trim shares with the
trim_kv_* functions reproduce the reference's index lists (tests/golden/g7_sparse.npz, g8_round2.npz), every refusal of
kvq_store_chunk_pool returns its code before any launch (ctypes with dummy pointers, never dereferenced), and trim /
keep_tokens / chunk_summarize reject bad arguments before they look at the store."""
import ctypes
import os

import pytest
import torch

from tests.conftest import load_golden

E_NULL, E_DIMS, E_DTYPE = -1, -2, -3
BIG = 1 << 31
NAME = "kvq_store_chunk_pool"
FAKE_IN, FAKE_SIN = ctypes.c_void_p(0x10000000), ctypes.c_void_p(0x20000000)  # 16-byte aligned, 256 MiB apart
FAKE_OUT, FAKE_SOUT = ctypes.c_void_p(0x30000000), ctypes.c_void_p(0x40000000)


@pytest.fixture(scope="module")
def lib():
    from efficient_llm_inference_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


# ---------------------------------------------------------------------------- shared index functions

def _expect(idx, T):
    return list(range(T)) if idx is None else idx


@pytest.mark.parametrize("T", (5, 40, 41, 100, 300, 1000))
@pytest.mark.parametrize("W,P", ((8, 0), (8, 4), (32, 3), (256, 32)))
def test_shared_index_functions_match_the_reference_lists(T, W, P):
    from efficient_llm_inference_amd.cache import implementations as I
    g7 = load_golden("g7_sparse.npz")
    assert _expect(I.keep_indices_prefix_window(T, P, W), T) == g7[f"prefix.T{T}.W{W}.P{P}"].tolist()
    for stride in (1, 3, 4):
        assert _expect(I.keep_indices_strided(T, W, stride, P), T) == g7[f"strided.T{T}.W{W}.P{P}.s{stride}"].tolist()
    for bs, kpb in ((16, 4), (64, 8), (7, 7)):
        assert _expect(I.keep_indices_block_old(T, W, bs, kpb, P), T) == g7[f"block.T{T}.W{W}.P{P}.b{bs}.k{kpb}"].tolist()
    for budget in (0, 1, 5, 64):
        assert _expect(I.keep_indices_budget_old(T, W, budget, P), T) == g7[f"budget.T{T}.W{W}.P{P}.n{budget}"].tolist()


def test_shared_index_functions_round2_edges():
    from efficient_llm_inference_amd.cache import implementations as I
    g8 = load_golden("g8_round2.npz")
    for T in (1, 7):
        assert _expect(I.keep_indices_sliding_window(T, 0), T) == g8[f"win0.T{T}"].tolist()
        for P in (0, 3):
            assert _expect(I.keep_indices_prefix_window(T, P, 0), T) == g8[f"prefix0.T{T}.P{P}"].tolist()
    for T in (97, 513, 2049, 4096, 16385, 32768):
        for (W, P, n) in ((8, 0, 7), (256, 32, 64), (33, 5, 100), (1, 1, 3)):
            assert _expect(I.keep_indices_budget_old(T, W, n, P), T) == g8[f"budget.T{T}.W{W}.P{P}.n{n}"].tolist(), (T, W, P, n)
    assert I.keep_indices_sliding_window(10, 4) == [6, 7, 8, 9] and I.keep_indices_sliding_window(4, 4) is None
    assert set(I.KEEP_INDEX_FNS) == {"sliding_window", "prefix_window", "strided", "block_old", "budget_old"}


def test_policy_names_and_defaults_are_those_of_the_fp16_functions():
    import inspect

    from efficient_llm_inference_amd.cache import implementations as I
    for policy, fn in I.KEEP_INDEX_FNS.items():
        ref = inspect.signature(getattr(I, "trim_kv_" + policy)).parameters
        got = inspect.signature(fn).parameters
        assert list(got)[0] == "T" and list(got)[-1] == "device"
        assert [(n, p.default) for n, p in list(got.items())[1:-1]] == [(n, p.default) for n, p in list(ref.items())[1:]], policy


# ---------------------------------------------------------------------------- kvq_store_chunk_pool refusals

def _dims(G=2, B=1, H=8, T=40, D=128):
    from efficient_llm_inference_amd._lib import KvqDims
    return KvqDims(G, B, H, T, D)


def _st(dm, T, row):
    from efficient_llm_inference_amd._lib import KvqStrides
    return KvqStrides(dm.B * dm.H * T * row, dm.H * T * row, T * row, row)


def _ref(x):
    return None if x is None else ctypes.byref(x)


def _call(lib, dm, bits=8, dtype=0, chunk_size=8, keep_last=4, eps=1e-8, **over):
    Dq = dm.D if bits == 8 else (dm.D + 1) // 2
    Tout = max(lib.kvq_chunk_summary_len(max(dm.T, 0), max(chunk_size, 1), max(keep_last, 0)), 1)
    a = dict(q_in=FAKE_IN, ist=_st(dm, max(dm.T, 1), Dq), s_in=FAKE_SIN, q_out=FAKE_OUT, ost=_st(dm, Tout, Dq), s_out=FAKE_SOUT, dims=dm)
    a.update(over)
    return lib.kvq_store_chunk_pool(bits, a["q_in"], _ref(a["ist"]), a["s_in"], max(dm.T, 1), a["q_out"], _ref(a["ost"]), a["s_out"],
                                    Tout, dtype, chunk_size, keep_last, eps, _ref(a["dims"]), None)


def _expect_rc(lib, rc, want, *needles):
    assert rc == want, rc
    msg = lib.kvq_last_error_string()
    assert NAME.encode() in msg, msg
    for n in needles:
        assert n in msg, msg


@pytest.mark.parametrize("null", ["q_in", "ist", "s_in", "q_out", "ost", "s_out", "dims"])
def test_store_pool_null_arguments(lib, null):
    _expect_rc(lib, _call(lib, _dims(), **{null: None}), E_NULL, b"NULL argument")
    if null != "dims":
        _expect_rc(lib, _call(lib, _dims(G=0), **{null: None}), E_NULL, b"NULL argument")  # before the empty return


@pytest.mark.parametrize("field", ["G", "B", "H", "T", "D"])
def test_store_pool_negative_dim(lib, field):
    dm = _dims()
    setattr(dm, field, -1)
    _expect_rc(lib, _call(lib, dm), E_DIMS, b"negative dim")


@pytest.mark.parametrize("big", [dict(T=BIG), dict(D=BIG), dict(B=1 << 16, H=1 << 15)])
def test_store_pool_dims_too_large(lib, big):
    _expect_rc(lib, _call(lib, _dims(**big)), E_DIMS, b"dims too large")


@pytest.mark.parametrize("bits", [0, 2, 16, -4])
def test_store_pool_bits(lib, bits):
    _expect_rc(lib, _call(lib, _dims(), bits=bits), E_DIMS, b"bits must be 8 or 4")
    _expect_rc(lib, _call(lib, _dims(G=0), bits=bits), E_DIMS, b"bits must be 8 or 4")


@pytest.mark.parametrize("dtype", [2, 3, -1])  # fp32 stores do not exist on this path
def test_store_pool_dtype(lib, dtype):
    _expect_rc(lib, _call(lib, _dims(), dtype=dtype), E_DTYPE, b"dtype must be KVQ_F16 or KVQ_BF16")
    _expect_rc(lib, _call(lib, _dims(), dtype=dtype, chunk_size=0), E_DTYPE, b"dtype must be")  # the dtype comes first


@pytest.mark.parametrize("own", [dict(chunk_size=0), dict(chunk_size=-4), dict(keep_last=-1), dict(chunk_size=BIG)])
@pytest.mark.parametrize("bits", [8, 4])
def test_store_pool_own_parameters(lib, own, bits):
    _expect_rc(lib, _call(lib, _dims(), bits=bits, **own), E_DIMS, b"chunk_size must be > 0 and keep_last >= 0")
    _expect_rc(lib, _call(lib, _dims(G=0), bits=bits, **own), E_DIMS, b"chunk_size must be")  # before the empty return


@pytest.mark.parametrize("shape", [dict(B=65, H=1, D=128), dict(B=1, H=8, D=1032), dict(B=8, H=8, D=129)])
def test_store_pool_slice_too_large(lib, shape):
    _expect_rc(lib, _call(lib, _dims(**shape)), E_DIMS, b"exceeds the 8192", b"kvq_chunk_meanpool")
    _expect_rc(lib, _call(lib, _dims(T=0, **shape)), E_DIMS, b"exceeds the 8192")  # before the empty return


@pytest.mark.parametrize("field", ["G", "B", "H", "T", "D"])
def test_store_pool_empty_launches_nothing(lib, field):
    dm = _dims()
    setattr(dm, field, 0)
    assert _call(lib, dm) == 0 and _call(lib, dm, bits=4, dtype=1) == 0


@pytest.mark.parametrize("bits", [8, 4])
def test_store_pool_overlap(lib, bits):
    dm = _dims()
    Dq = dm.D if bits == 8 else dm.D // 2
    n_in = dm.G * dm.B * dm.H * dm.T * Dq
    for q_out in (FAKE_IN, ctypes.c_void_p(FAKE_IN.value + n_in - 16), ctypes.c_void_p(FAKE_IN.value - 16)):
        _expect_rc(lib, _call(lib, dm, bits=bits, q_out=q_out), E_DIMS, b"overlap")
    for s_out in (FAKE_SIN, ctypes.c_void_p(FAKE_SIN.value + 4 * (dm.G * dm.T - 1)), ctypes.c_void_p(FAKE_SIN.value - 4)):
        _expect_rc(lib, _call(lib, dm, bits=bits, s_out=s_out), E_DIMS, b"overlap")


def test_store_pool_tunable(lib):
    assert lib.kvq_get_tunable(b"store_pool_fast") == 1
    assert lib.kvq_set_tunable(b"store_pool_fast", 0) == 0 and lib.kvq_get_tunable(b"store_pool_fast") == 0
    assert lib.kvq_set_tunable(b"store_pool_fast", 1) == 0


# ---------------------------------------------------------------------------- the Python surface, before any store access

def _cache():
    import efficient_llm_inference_amd as E
    return E.QuantizedKVCache(2, "mixed", device="cpu")


def test_trim_rejects_unknown_policies_and_bad_arguments():
    qc = _cache()
    for policy in ("chunk_summary", "window", "", None):
        with pytest.raises(ValueError, match="unknown eviction policy"):
            qc.trim(policy, 4)
    with pytest.raises(ValueError, match="must be >= 0"):
        qc.trim("sliding_window", -1)
    with pytest.raises(ValueError, match="must be >= 0"):
        qc.trim("strided", window_size=4, stride=2, prefix_len=-3)
    with pytest.raises(TypeError, match="must be an int"):
        qc.trim("strided", 4.0, 2)
    with pytest.raises(TypeError, match="must be an int"):
        qc.trim("budget_old", window_size=4, old_budget=True)
    with pytest.raises(TypeError):
        qc.trim("strided", 4, 2, device="cpu")
    with pytest.raises(ValueError, match="Empty cache"):  # valid arguments reach the store
        qc.trim("strided", 4, 2)


def test_chunk_summarize_and_keep_tokens_reject_bad_arguments():
    qc = _cache()
    for args in ((0, 4), (-1, 4), (8, -1)):
        with pytest.raises(ValueError, match="chunk_size must be > 0 and keep_last >= 0"):
            qc.chunk_summarize(*args)
    with pytest.raises(TypeError):
        qc.chunk_summarize(8.5, 4)
    with pytest.raises(ValueError, match="Empty cache"):
        qc.chunk_summarize(8, 4)
    with pytest.raises(ValueError, match="Empty cache"):
        qc.keep_tokens([0])
    with pytest.raises(ValueError, match="different token counts|same number of tokens"):
        qc._k.lens[0] = 3
        qc.keep_tokens([0])


def test_benchmarker_quant_eviction_refuses_the_fused_paths():
    from efficient_llm_inference_amd.benchmarking.benchmarker import KVCacheBenchmarker

    class Tok:
        def __call__(self, prompt, return_tensors="pt", **kw):
            return type("E", (), {"input_ids": torch.zeros(1, 4, dtype=torch.long)})()

    bm = KVCacheBenchmarker(model=None, tokenizer=Tok(), device="cpu")
    assert bm.quant_eviction is None
    bm.quant_eviction = ("strided", dict(window_size=4, stride=2))
    for flags in (dict(fused_attention=True), dict(fused_attention=True, graph_decode=True)):
        for k, v in flags.items():
            setattr(bm, k, v)
        with pytest.raises(RuntimeError, match="quant_eviction does not combine"):
            bm.generate_with_quantized_kv("x", 2, "int8")
