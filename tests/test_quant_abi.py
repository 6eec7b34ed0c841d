"""Return codes of the five quantise entry points for every validation branch (no GPU needed: each case returns before
any launch, so fake device pointers are never dereferenced).

The two families check in different orders, and both orders are pinned: kvq_quant_i8/i4_tokens return 0 for an empty
slice before they look at "dims too large"; the split-phase entry points (kvq_absmax_tokens[_acc],
kvq_quant_tokens_from_absmax) check the dims first."""
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


def _dims(G=1, B=1, H=8, T=1, D=128):
    from efficient_llm_inference_amd._lib import KvqDims
    return KvqDims(G, B, H, T, D)


def _st(dm, last):
    """contiguous [G,B,H,T,last] strides (elements for an input, bytes for an int8 store)"""
    from efficient_llm_inference_amd._lib import KvqStrides
    return KvqStrides(dm.B * dm.H * dm.T * last, dm.H * dm.T * last, dm.T * last, last)


def _ptrs(*ps):
    return (ctypes.c_void_p * len(ps))(*[p.value if p is not None else None for p in ps])


# one caller per entry point: (lib, dims, in_base, in_ptrs, dtype, null, workspace, bits) -> rc
def _quant(bits):
    def call(lib, dm, base=FAKE, ptrs=None, dtype=0, null=False, ws=FAKE, b=None):
        from efficient_llm_inference_amd._lib import byref
        fn = lib.kvq_quant_i8_tokens if bits == 8 else lib.kvq_quant_i4_tokens
        ist, qst = _st(dm, dm.D), _st(dm, dm.D * bits // 8)
        return fn(base, ptrs, byref(ist), dtype, None if null else FAKE, byref(qst), FAKE, 1, ws, 1e-8, byref(dm), None)
    return call


def _absmax(acc):
    def call(lib, dm, base=FAKE, ptrs=None, dtype=0, null=False, ws=FAKE, b=None):
        from efficient_llm_inference_amd._lib import byref
        fn = lib.kvq_absmax_tokens_acc if acc else lib.kvq_absmax_tokens
        return fn(base, ptrs, byref(_st(dm, dm.D)), dtype, None if null else FAKE, byref(dm), None)
    return call


def _from_absmax(lib, dm, base=FAKE, ptrs=None, dtype=0, null=False, ws=FAKE, b=8):
    from efficient_llm_inference_amd._lib import byref
    ist, qst = _st(dm, dm.D), _st(dm, dm.D)
    return lib.kvq_quant_tokens_from_absmax(b, base, ptrs, byref(ist), dtype, None if null else FAKE, byref(qst), FAKE, 1,
                                            FAKE, 1e-8, byref(dm), None)


ENTRIES = {
    "kvq_quant_i8_tokens": _quant(8),
    "kvq_quant_i4_tokens": _quant(4),
    "kvq_absmax_tokens": _absmax(False),
    "kvq_absmax_tokens_acc": _absmax(True),
    "kvq_quant_tokens_from_absmax": _from_absmax,
}
SPLIT = ("kvq_absmax_tokens", "kvq_absmax_tokens_acc", "kvq_quant_tokens_from_absmax")


def _expect(lib, name, rc, want, *needles):
    assert rc == want, (name, rc)
    if want != 0:
        msg = lib.kvq_last_error_string()
        assert name.encode() in msg, msg
        for n in needles:
            assert n in msg, msg


@pytest.mark.parametrize("name", list(ENTRIES))
def test_null_arguments(lib, name):
    call = ENTRIES[name]
    _expect(lib, name, call(lib, _dims(), null=True), E_NULL, b"NULL")  # output (store / table) missing
    _expect(lib, name, call(lib, _dims(), base=None), E_NULL, b"NULL")  # neither in_base nor in_ptrs
    from efficient_llm_inference_amd._lib import byref
    if name == "kvq_quant_tokens_from_absmax":
        rc = lib.kvq_quant_tokens_from_absmax(8, FAKE, None, byref(_st(_dims(), 128)), 0, FAKE, None, FAKE, 1, FAKE, 1e-8,
                                              byref(_dims()), None)  # no store strides
    elif name in SPLIT:
        rc = getattr(lib, name)(FAKE, None, None, 0, FAKE, byref(_dims()), None)  # no input strides
    else:
        rc = getattr(lib, name)(FAKE, None, byref(_st(_dims(), 128)), 0, FAKE, byref(_st(_dims(), 128)), None, 1, FAKE, 1e-8,
                                byref(_dims()), None)  # no scale table
    _expect(lib, name, rc, E_NULL, b"NULL")


@pytest.mark.parametrize("name", list(ENTRIES))
def test_in_base_and_in_ptrs_both_given(lib, name):
    _expect(lib, name, ENTRIES[name](lib, _dims(), ptrs=_ptrs(FAKE)), E_DIMS)


@pytest.mark.parametrize("name", list(ENTRIES))
@pytest.mark.parametrize("field", ["G", "B", "H", "T", "D"])
def test_negative_dim(lib, name, field):
    dm = _dims()
    setattr(dm, field, -1)
    _expect(lib, name, ENTRIES[name](lib, dm), E_DIMS)
    dm.G = 0  # negative dims are refused before the empty-slice shortcut, in every entry point
    if field != "G":
        _expect(lib, name, ENTRIES[name](lib, dm), E_DIMS)


@pytest.mark.parametrize("name", list(ENTRIES))
def test_unknown_dtype(lib, name):
    _expect(lib, name, ENTRIES[name](lib, _dims(), dtype=7), E_DTYPE)
    _expect(lib, name, ENTRIES[name](lib, _dims(G=0), dtype=3), E_DTYPE)  # before the empty-slice shortcut


@pytest.mark.parametrize("bits", [0, 2, 5, 16])
def test_from_absmax_bits(lib, bits):
    name = "kvq_quant_tokens_from_absmax"
    _expect(lib, name, _from_absmax(lib, _dims(), b=bits), E_DIMS)
    _expect(lib, name, _from_absmax(lib, _dims(G=0), b=bits), E_DIMS)  # before the empty-slice shortcut
    _expect(lib, name, _from_absmax(lib, _dims(), b=bits, dtype=7), E_DTYPE)  # after the dtype


@pytest.mark.parametrize("name", list(ENTRIES))
@pytest.mark.parametrize("field", ["G", "B", "H", "T", "D"])
def test_empty_slice_launches_nothing(lib, name, field):
    dm = _dims()
    setattr(dm, field, 0)
    assert ENTRIES[name](lib, dm, ws=None) == 0


@pytest.mark.parametrize("name", list(ENTRIES))
@pytest.mark.parametrize("big", [dict(B=BIG), dict(H=BIG), dict(T=BIG), dict(D=BIG), dict(B=1 << 16, H=1 << 15)])
def test_dims_too_large(lib, name, big):
    _expect(lib, name, ENTRIES[name](lib, _dims(**big)), E_DIMS)
    # an empty slice with a dim that is too large: the quantise entry points return 0 first, the split phases refuse it
    rc = ENTRIES[name](lib, _dims(G=0, **big))
    if name in SPLIT:
        _expect(lib, name, rc, E_DIMS, b"bad dims")
    else:
        assert rc == 0


@pytest.mark.parametrize("name", ["kvq_quant_i8_tokens", "kvq_quant_i4_tokens"])
@pytest.mark.parametrize("D", [7, 127])
def test_odd_head_dim_needs_the_workspace(lib, name, D):
    _expect(lib, name, ENTRIES[name](lib, _dims(D=D), ws=None), E_NULL)


@pytest.mark.parametrize("name", list(ENTRIES))
@pytest.mark.parametrize("D", [128, 7])
def test_null_entry_in_ptrs(lib, name, D):
    # reported by the launch-chunk loop: no path before it takes a NULL group pointer
    _expect(lib, name, ENTRIES[name](lib, _dims(G=2, D=D), base=None, ptrs=_ptrs(FAKE, None)), E_NULL, b"NULL")
    _expect(lib, name, ENTRIES[name](lib, _dims(G=2, D=D), base=None, ptrs=_ptrs(None, FAKE)), E_NULL, b"NULL")
