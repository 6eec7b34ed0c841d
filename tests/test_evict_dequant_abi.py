"""Return codes of the eviction and dequantise entry points for every validation branch (no GPU needed: each case returns
before any launch, so fake device pointers are never dereferenced).

The order of the checks is pinned too. The three eviction entry points share their first four (NULL arguments, in_base
and in_ptrs both given, a negative dim, a dim >= 2^31), all of which precede the empty-slice return; each then checks its
own parameters, still before the empty return, and only then meets what the launch-chunk loop refuses (a NULL entry in
in_ptrs, too many segments / elements). kvq_chunk_meanpool looks at the dtype before chunk_size. The dequantise *_tokens
pair checks NULL, negative dims, out_dtype, empty, in that order; the flat pair sizes, empty, NULL."""
import ctypes
import os

import pytest

E_NULL, E_DIMS, E_DTYPE = -1, -2, -3
BIG = 1 << 31
FAKE = ctypes.c_void_p(0x1000)  # 16-byte aligned, never dereferenced


@pytest.fixture(scope="module")
def lib():
    from efficient_llm_inference_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _dims(G=1, B=1, H=8, T=4, D=128):
    from efficient_llm_inference_amd._lib import KvqDims
    return KvqDims(G, B, H, T, D)


def _st(dm, last, t=None):
    """contiguous [G,B,H,T,last] strides; t: another token stride"""
    from efficient_llm_inference_amd._lib import KvqStrides
    return KvqStrides(dm.B * dm.H * dm.T * last, dm.H * dm.T * last, dm.T * last, last if t is None else t)


def _ptrs(*ps):
    return (ctypes.c_void_p * len(ps))(*[p.value if p is not None else None for p in ps])


def _ref(x):
    return None if x is None else ctypes.byref(x)


def _expect(lib, name, rc, want, *needles):
    assert rc == want, (name, rc)
    if want != 0:
        msg = lib.kvq_last_error_string()
        assert name.encode() in msg, msg
        for n in needles:
            assert n in msg, msg


# ---------------------------------------------------------------------------- eviction
# one caller per entry point; `own` are the entry point's own parameters between out_st and dims
EVICT_OWN = {
    "kvq_window_compact": dict(elem_size=2, window=2),
    "kvq_gather_tokens": dict(elem_size=2, idx=FAKE, n_idx=2),
    "kvq_chunk_meanpool": dict(dtype=0, chunk_size=2, keep_last=1),
}


def _evict(lib, name, dm, base=FAKE, ptrs=None, ist="contig", ost="contig", out=FAKE, **own):
    kw = dict(EVICT_OWN[name], **own)
    ist = _st(dm, dm.D) if ist == "contig" else ist
    ost = _st(dm, dm.D) if ost == "contig" else ost
    return getattr(lib, name)(base, ptrs, _ref(ist), out, _ref(ost), *kw.values(), _ref(dm), None)


EVICT = list(EVICT_OWN)


@pytest.mark.parametrize("name", EVICT)
def test_evict_null_arguments(lib, name):
    for missing in (dict(ist=None), dict(ost=None), dict(out=None), dict(base=None)):
        _expect(lib, name, _evict(lib, name, _dims(), **missing), E_NULL, b"NULL argument")
    kw = EVICT_OWN[name]
    rc = getattr(lib, name)(FAKE, None, _ref(_st(_dims(), 128)), FAKE, _ref(_st(_dims(), 128)), *kw.values(), None, None)
    _expect(lib, name, rc, E_NULL, b"NULL argument")  # no dims


@pytest.mark.parametrize("name", EVICT)
def test_evict_in_base_and_in_ptrs_both_given(lib, name):
    _expect(lib, name, _evict(lib, name, _dims(), ptrs=_ptrs(FAKE)), E_DIMS, b"not both")


@pytest.mark.parametrize("name", EVICT)
@pytest.mark.parametrize("field", ["G", "B", "H", "T", "D"])
def test_evict_negative_dim(lib, name, field):
    dm = _dims()
    setattr(dm, field, -1)
    _expect(lib, name, _evict(lib, name, dm), E_DIMS, b"negative dim")
    if field != "G":
        dm.G = 0  # before the empty return
        _expect(lib, name, _evict(lib, name, dm), E_DIMS, b"negative dim")


@pytest.mark.parametrize("name", EVICT)
@pytest.mark.parametrize("big", [dict(T=BIG), dict(D=BIG), dict(B=1 << 16, H=1 << 15), dict(B=BIG, H=1)])
def test_evict_dims_too_large(lib, name, big):
    _expect(lib, name, _evict(lib, name, _dims(**big)), E_DIMS, b"dims too large")
    _expect(lib, name, _evict(lib, name, _dims(G=0, **big)), E_DIMS, b"dims too large")  # before the empty return


@pytest.mark.parametrize("name", EVICT)
def test_evict_null_entry_in_ptrs(lib, name):
    for ptrs, i in ((_ptrs(FAKE, None), b"in_ptrs[1]"), (_ptrs(None, FAKE), b"in_ptrs[0]")):
        _expect(lib, name, _evict(lib, name, _dims(G=2), base=None, ptrs=ptrs), E_NULL, i, b"is NULL")


@pytest.mark.parametrize("name", EVICT)
@pytest.mark.parametrize("field", ["G", "B", "H", "T", "D"])
def test_evict_empty_launches_nothing(lib, name, field):
    dm, own = _dims(), {}
    if name == "kvq_gather_tokens" and field == "T":
        own = dict(n_idx=0)  # its output has n_idx tokens, whatever T is (T = 0: rows of zeros)
    else:
        setattr(dm, field, 0)
    assert _evict(lib, name, dm, **own) == 0
    assert _evict(lib, name, dm, base=None, ptrs=_ptrs(None), **own) == 0  # never looks at the pointer table


@pytest.mark.parametrize("own", [dict(elem_size=3), dict(elem_size=0), dict(elem_size=8), dict(window=-1)])
def test_window_compact_own_parameters(lib, own):
    name = "kvq_window_compact"
    _expect(lib, name, _evict(lib, name, _dims(), **own), E_DIMS, b"elem_size must be 2 or 4 and window >= 0")
    _expect(lib, name, _evict(lib, name, _dims(T=0), **own), E_DIMS, b"elem_size must be")  # before the empty return
    _expect(lib, name, _evict(lib, name, _dims(T=BIG), **own), E_DIMS, b"dims too large")  # after the shared checks


def test_window_compact_zero_window(lib):
    assert _evict(lib, "kvq_window_compact", _dims(), window=0) == 0
    assert _evict(lib, "kvq_window_compact", _dims(), window=0, elem_size=4) == 0


@pytest.mark.parametrize("elem_size", [2, 4])
def test_window_compact_too_many_segments(lib, elem_size):
    # strided tokens: one segment per kept token, B*H * W * 1 chunk = 2^31 workgroups
    name = "kvq_window_compact"
    dm = _dims(B=1 << 15, H=1 << 15, T=2, D=8)
    _expect(lib, name, _evict(lib, name, dm, ist=_st(dm, 8, t=16), window=2, elem_size=elem_size), E_DIMS,
            b"too many segments")
    _expect(lib, name, _evict(lib, name, dm, ost=_st(dm, 8, t=16), window=5, elem_size=elem_size), E_DIMS,
            b"too many segments")  # W = min(window, T)
    # refused before the pointer table is read
    _expect(lib, name, _evict(lib, name, dm, ist=_st(dm, 8, t=16), base=None, ptrs=_ptrs(None)), E_DIMS, b"too many segments")


@pytest.mark.parametrize("own,needle", [(dict(elem_size=3), b"elem_size must be 2 or 4"), (dict(n_idx=-1), b"n_idx < 2^31"),
                                        (dict(n_idx=BIG), b"n_idx < 2^31")])
def test_gather_own_parameters(lib, own, needle):
    name = "kvq_gather_tokens"
    _expect(lib, name, _evict(lib, name, _dims(), **own), E_DIMS, needle)
    _expect(lib, name, _evict(lib, name, _dims(G=0), **own), E_DIMS, needle)  # before the empty return
    _expect(lib, name, _evict(lib, name, _dims(D=BIG), **own), E_DIMS, b"dims too large")  # after the shared checks


def test_gather_idx_null(lib):
    name = "kvq_gather_tokens"
    assert _evict(lib, name, _dims(), idx=None, n_idx=0) == 0
    assert _evict(lib, name, _dims(G=0), idx=None) == 0
    _expect(lib, name, _evict(lib, name, _dims(), idx=None), E_NULL, b"idx is NULL")
    # idx comes before the pointer table
    _expect(lib, name, _evict(lib, name, _dims(), idx=None, base=None, ptrs=_ptrs(None)), E_NULL, b"idx is NULL")


@pytest.mark.parametrize("elem_size,D", [(2, 8), (2, 7), (4, 4)])
def test_gather_too_many_elements(lib, elem_size, D):
    # 2^20 (b, h) rows x 2^20 indices x at least one piece each >= 2^32 work items, vector route (D 8) or scalar
    name = "kvq_gather_tokens"
    dm = _dims(B=1 << 10, H=1 << 10, T=4, D=D)
    _expect(lib, name, _evict(lib, name, dm, n_idx=1 << 20, elem_size=elem_size), E_DIMS, b"too many elements per group")
    # the pointer table is read first
    _expect(lib, name, _evict(lib, name, dm, n_idx=1 << 20, elem_size=elem_size, base=None, ptrs=_ptrs(None)), E_NULL,
            b"in_ptrs[0] is NULL")


def test_meanpool_dtype_before_chunk_size(lib):
    name = "kvq_chunk_meanpool"
    _expect(lib, name, _evict(lib, name, _dims(), dtype=7, chunk_size=0), E_DTYPE, b"unknown dtype 7")
    _expect(lib, name, _evict(lib, name, _dims(G=0), dtype=3), E_DTYPE, b"unknown dtype 3")  # before the empty return
    _expect(lib, name, _evict(lib, name, _dims(), dtype=-1), E_DTYPE, b"unknown dtype")
    _expect(lib, name, _evict(lib, name, _dims(T=BIG), dtype=7), E_DIMS, b"dims too large")  # after the shared checks


@pytest.mark.parametrize("own", [dict(chunk_size=0), dict(chunk_size=-4), dict(keep_last=-1), dict(chunk_size=BIG)])
@pytest.mark.parametrize("dtype", [0, 1, 2])
def test_meanpool_own_parameters(lib, own, dtype):
    name = "kvq_chunk_meanpool"
    _expect(lib, name, _evict(lib, name, _dims(), dtype=dtype, **own), E_DIMS, b"chunk_size must be > 0 and keep_last >= 0")
    _expect(lib, name, _evict(lib, name, _dims(G=0), dtype=dtype, **own), E_DIMS, b"chunk_size must be")


# ---------------------------------------------------------------------------- dequantise, token tables
DEQ_TOKENS = ["kvq_dequant_i8_tokens", "kvq_dequant_i4_tokens"]


def _deq(lib, name, dm, out_dtype=0, null=None):
    """null: which of the six pointers (q, q_st, scales, out, out_st, dims) is missing"""
    Dq = dm.D if "i8" in name else (dm.D + 1) // 2
    a = dict(q=FAKE, q_st=_ref(_st(dm, Dq)), scales=FAKE, out=FAKE, out_st=_ref(_st(dm, dm.D)), dims=_ref(dm))
    if null:
        a[null] = None
    return getattr(lib, name)(a["q"], a["q_st"], a["scales"], dm.T, a["out"], a["out_st"], out_dtype, a["dims"], None)


@pytest.mark.parametrize("name", DEQ_TOKENS)
@pytest.mark.parametrize("null", ["q", "q_st", "scales", "out", "out_st", "dims"])
def test_dequant_tokens_null_arguments(lib, name, null):
    _expect(lib, name, _deq(lib, name, _dims(), null=null), E_NULL, b"NULL argument")
    if null != "dims":
        _expect(lib, name, _deq(lib, name, _dims(G=0), null=null), E_NULL, b"NULL argument")  # before the empty return
        _expect(lib, name, _deq(lib, name, _dims(T=-1), out_dtype=7, null=null), E_NULL, b"NULL argument")  # first


@pytest.mark.parametrize("name", DEQ_TOKENS)
@pytest.mark.parametrize("field", ["G", "B", "H", "T", "D"])
def test_dequant_tokens_negative_dim(lib, name, field):
    dm = _dims()
    setattr(dm, field, -1)
    _expect(lib, name, _deq(lib, name, dm), E_DIMS, b"negative dim")
    _expect(lib, name, _deq(lib, name, dm, out_dtype=7), E_DIMS, b"negative dim")  # before the dtype
    if field != "G":
        dm.G = 0
        _expect(lib, name, _deq(lib, name, dm), E_DIMS, b"negative dim")


@pytest.mark.parametrize("name", DEQ_TOKENS)
def test_dequant_tokens_unknown_dtype(lib, name):
    _expect(lib, name, _deq(lib, name, _dims(), out_dtype=7), E_DTYPE, b"unknown out_dtype 7")
    _expect(lib, name, _deq(lib, name, _dims(G=0), out_dtype=3), E_DTYPE, b"unknown out_dtype 3")  # before the empty return
    _expect(lib, name, _deq(lib, name, _dims(), out_dtype=-1), E_DTYPE, b"unknown out_dtype")


@pytest.mark.parametrize("name", DEQ_TOKENS)
@pytest.mark.parametrize("field", ["G", "B", "H", "T", "D"])
@pytest.mark.parametrize("out_dtype", [0, 1, 2])
def test_dequant_tokens_empty_launches_nothing(lib, name, field, out_dtype):
    dm = _dims()
    setattr(dm, field, 0)
    assert _deq(lib, name, dm, out_dtype=out_dtype) == 0


@pytest.mark.parametrize("name", DEQ_TOKENS)
@pytest.mark.parametrize("big", [dict(T=1 << 32, D=1), dict(T=1, D=(1 << 32) + 1), dict(B=1 << 16, H=1 << 16, T=1, D=3)])
@pytest.mark.parametrize("out_dtype", [0, 1, 2])
def test_dequant_tokens_generic_dims_too_large(lib, name, big, out_dtype):
    # head dims that are no multiple of 8 take the generic kernel, whose 32-bit fields these do not fit
    dm = _dims(**dict(dict(B=1, H=1), **big))
    _expect(lib, name, _deq(lib, name, dm, out_dtype=out_dtype), E_DIMS, b"dims too large for the generic path")


# ---------------------------------------------------------------------------- dequantise, flat buffers
def test_dequant_i8_flat(lib):
    name = "kvq_dequant_i8_f16_flat"
    f = lib.kvq_dequant_i8_f16_flat
    _expect(lib, name, f(FAKE, 1.0, FAKE, -1, None), E_DIMS, b"n < 0")
    _expect(lib, name, f(None, 1.0, None, -8, None), E_DIMS, b"n < 0")  # sizes before NULL
    assert f(None, 1.0, None, 0, None) == 0  # empty before NULL
    for n in (8, 7, 1 << 24):  # vector, scalar and chunk sizes
        _expect(lib, name, f(None, 1.0, FAKE, n, None), E_NULL, b"NULL argument")
        _expect(lib, name, f(FAKE, 1.0, None, n, None), E_NULL, b"NULL argument")


def test_dequant_i4_flat(lib):
    name = "kvq_dequant_i4_f16_flat"
    f = lib.kvq_dequant_i4_f16_flat
    for sizes in ((-1, 4, 8), (8, -1, 8), (8, 4, -1), (10, 4, 8), (4, 8, 16)):  # the last two: n_packed % packed_last != 0
        _expect(lib, name, f(FAKE, 1.0, FAKE, *sizes, None), E_DIMS, b"bad sizes", b"n_packed=%d" % sizes[0],
                b"packed_last=%d" % sizes[1], b"orig_last_dim=%d" % sizes[2])
        _expect(lib, name, f(None, 1.0, None, *sizes, None), E_DIMS, b"bad sizes")  # sizes before NULL
    assert f(None, 1.0, None, 0, 4, 8, None) == 0  # empty before NULL
    assert f(None, 1.0, None, 0, 0, 0, None) == 0
    for sizes in ((8, 4, 8), (8, 4, 7), (6, 3, 6), (1 << 23, 64, 128)):  # vector, pad column, scalar, chunk
        _expect(lib, name, f(None, 1.0, FAKE, *sizes, None), E_NULL, b"NULL argument")
        _expect(lib, name, f(FAKE, 1.0, None, *sizes, None), E_NULL, b"NULL argument")
