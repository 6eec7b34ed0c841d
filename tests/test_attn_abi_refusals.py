"""The C-level refusals of the thirteen attention entry points (ten decode, three extend) and the two decode workspace
functions, as a table of (entry point, arguments, return code, message substring) driven through ctypes. No row launches
anything: the pointers are never dereferenced (a fake address on the host, one small device buffer on the GPU), and the
kernel log is empty afterwards. What the table pins is the order of the checks, the codes, the message texts and the entry
point's name in them — what a rewritten forwarding layer can break without any kernel noticing.

Rows that the host reaches before it asks the runtime about a pointer run without a GPU; the decode rows behind the device
check of ``out`` carry the ``gpu`` marker."""
import ctypes

import pytest

E_NULL, E_DIMS, E_DTYPE = -1, -2, -3
F16, F32 = 0, 2
FAKE = 0x1000  # 16-byte aligned, never dereferenced
BIG = 1 << 40  # workspace floats no plan exceeds

DECODE_ATTN = ("kvq_decode_attn", "kvq_decode_attn_window", "kvq_decode_attn_padded")
DECODE_STEP = ("kvq_decode_step", "kvq_decode_step_window", "kvq_decode_step_padded")
DECODE_STEP_DEV = ("kvq_decode_step_dev", "kvq_decode_step_dev_window", "kvq_decode_step_dev_padded")
EXTEND = ("kvq_extend_attn", "kvq_extend_attn_window", "kvq_extend_attn_padded")
WINDOWED = tuple(n for fam in (DECODE_ATTN, DECODE_STEP, DECODE_STEP_DEV, EXTEND) for n in fam[1:])


@pytest.fixture(scope="module")
def lib():
    import os

    from efficient_llm_inference_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _defaults(entry, base):
    """A call of ``entry`` that passes every check (it would launch): decode dims (1, 8, 8, 256, 128), extend dims
    (1, 8, 8, 1024, 1, 128) whose plan takes several splits and so needs a workspace. ``base``: the address every pointer gets."""
    a = dict(q=base, q_s=(1024, 128, 128), k_store=base, k_st=(0, 1 << 20, 1 << 17, 128), k_scales=base, k_bits=8,
             v_store=base, v_st=(0, 1 << 20, 1 << 17, 128), v_scales=base, v_bits=8, k_new=base, kn_s=(1024, 128, 128),
             v_new=base, vn_s=(1024, 128, 128), out=base, o_s=(1024, 128, 128), dtype=F16, sm_scale=0.088, window=0,
             kv_start=base if entry.endswith("_padded") else None, eps=1e-8, ws=base, ws_floats=BIG, t_dev=base,
             dims=(1, 8, 8, 1024, 1, 128) if entry in EXTEND else (1, 8, 8, 256, 128))
    return a


def _call(lib, entry, base=FAKE, **over):
    from efficient_llm_inference_amd._lib import KvqAttnDims, KvqExtendDims, KvqStrides, byref
    a = _defaults(entry, base)
    unknown = set(over) - set(a)
    assert not unknown, unknown
    a.update({k: base + 8 if v == "off8" else v for k, v in over.items()})  # "off8": an address 8 bytes past a 16-byte boundary
    P = lambda v: None if v is None else ctypes.c_void_p(v)
    ext = entry in EXTEND
    ns = 3 if ext else 2  # strides per [B, H, (S,) D] tensor
    ten = lambda p, s: (P(a[p]),) + tuple(a[s][:ns])
    store = lambda w: (P(a[w + "_store"]), None if a[w + "_st"] is None else byref(KvqStrides(*a[w + "_st"])),
                       P(a[w + "_scales"]), a[w + "_bits"])
    dims = None if a["dims"] is None else byref((KvqExtendDims if ext else KvqAttnDims)(*a["dims"]))
    win = (a["window"], P(a["kv_start"])) if entry.endswith("_padded") else (a["window"],) if entry.endswith("_window") else ()
    tail = (P(a["ws"]), a["ws_floats"], dims)
    if ext or entry in DECODE_ATTN:
        args = ten("q", "q_s") + store("k") + store("v") + ten("k_new", "kn_s") + ten("v_new", "vn_s") + ten("out", "o_s") + \
            (a["dtype"], a["sm_scale"]) + win + tail
    else:
        args = ten("q", "q_s") + ten("k_new", "kn_s") + ten("v_new", "vn_s") + store("k") + store("v") + ten("out", "o_s") + \
            (a["dtype"], a["sm_scale"]) + win + (a["eps"],) + tail
        if entry in DECODE_STEP_DEV:
            args += (P(a["t_dev"]),)
    rc = getattr(lib, entry)(*args, None)
    return rc, lib.kvq_last_error_string().decode()


def _name(entry, over):
    """the name an entry point reports: a ``_padded`` call without kv_start is the ``_window`` call"""
    if entry.endswith("_padded") and "kv_start" in over and over["kv_start"] is None:
        return entry.replace("_padded", "_window")
    return entry


def _rows(table):
    return [pytest.param(e, o, rc, msg, id=f"{e}-{msg[:28].strip().replace(' ', '_')}-{i}") for i, (e, o, rc, msg) in enumerate(table)]


# ---------------------------------------------------------------------------------------------------------------- host rows
HOST = []
for e in EXTEND:
    HOST += [
        (e, dict(q=None), E_NULL, "NULL q / k_new / v_new / out / dims"),
        (e, dict(k_new=None), E_NULL, "NULL q / k_new / v_new / out / dims"),
        (e, dict(out=None), E_NULL, "NULL q / k_new / v_new / out / dims"),
        (e, dict(dims=None), E_NULL, "NULL q / k_new / v_new / out / dims"),
        (e, dict(dims=(1, 8, 8, 1024, 0, 128)), E_DIMS, "bad dims B=1 Hq=8 Hkv=8 T=1024 S=0 D=128: B, Hq, Hkv, S, D must be positive and T >= 0"),
        (e, dict(dims=(1, 8, 3, 1024, 1, 128)), E_DIMS, "need Hq % Hkv == 0 and Hq / Hkv <= 16"),
        (e, dict(dims=(1, 34, 2, 1024, 1, 128)), E_DIMS, "need Hq % Hkv == 0 and Hq / Hkv <= 16"),
        (e, dict(dims=(65536, 1, 1, 1024, 1, 128)), E_DIMS, "B * Hkv must stay below 65536"),
        (e, dict(dims=(1, 8, 8, 1 << 31, 1, 128)), E_DIMS, "T must stay below 2^31 and S below 2^24"),
        (e, dict(dims=(1, 8, 8, 1024, 1, 32)), E_DIMS, "head_dim must be 64 or 128"),
        (e, dict(dtype=F32), E_DTYPE, "dtype 2 not supported (KVQ_F16, KVQ_BF16)"),
        (e, dict(k_bits=3), E_DIMS, "k_bits / v_bits must be 8 or 4"),
        (e, dict(v_bits=16), E_DIMS, "k_bits / v_bits must be 8 or 4"),
        (e, dict(k_store=None), E_NULL, "NULL store / scales / strides"),
        (e, dict(v_scales=None), E_NULL, "NULL store / scales / strides"),
        (e, dict(k_st=None), E_NULL, "NULL store / scales / strides"),
        (e, dict(ws_floats=16), E_DIMS, "workspace of 16 floats, 532480 needed"),
        (e, dict(ws=None), E_NULL, "workspace of 0 floats, 532480 needed"),
        (e, dict(ws="off8"), E_DIMS, "workspace must be 16-byte aligned"),
        (e, dict(k_store="off8"), E_DIMS, "store rows must be 16 / 16 byte aligned"),
        (e, dict(v_bits=4, v_st=(0, 1 << 20, 1 << 17, 68)), E_DIMS, "store rows must be 16 / 8 byte aligned"),
        (e, dict(k_st=(0, 1 << 20, 1 << 17, 64)), E_DIMS, "store token stride shorter than a row"),
        (e, dict(q="off8"), E_DIMS, "q / k_new / v_new / out must be 16-byte aligned with strides that are multiples of 8 elements"),
        (e, dict(vn_s=(1024, 132, 128)), E_DIMS, "q / k_new / v_new / out must be 16-byte aligned with strides that are multiples of 8 elements"),
        (e, dict(o_s=(1024, 128, 4)), E_DIMS, "q / k_new / v_new / out must be 16-byte aligned with strides that are multiples of 8 elements"),
    ]
for e in DECODE_ATTN:
    HOST += [
        (e, dict(q=None), E_NULL, "NULL q / out / dims"),
        (e, dict(out=None), E_NULL, "NULL q / out / dims"),
        (e, dict(dims=None), E_NULL, "NULL q / out / dims"),
    ]
for e in DECODE_STEP + DECODE_STEP_DEV:
    HOST += [
        (e, dict(k_new=None), E_NULL, "NULL argument"),
        (e, dict(v_scales=None), E_NULL, "NULL argument"),
        (e, dict(ws=None), E_NULL, "NULL argument"),
        (e, dict(dims=None), E_NULL, "NULL argument"),
        (e, dict(q=None), E_NULL, "NULL q / out / dims"),  # past the step's own checks, refused by the shared body
        (e, dict(out=None), E_NULL, "NULL q / out / dims"),
    ]
HOST += [(e, dict(t_dev=None), E_NULL, "NULL argument") for e in DECODE_STEP_DEV]
HOST += [(e, dict(window=-1), E_DIMS, "window -1 must be >= 0 (0 = none)") for e in WINDOWED]
# a padded entry point without kv_start is the windowed call, and says so
HOST += [(e, dict(window=-3, kv_start=None), E_DIMS, "window -3 must be >= 0 (0 = none)") for e in WINDOWED if e.endswith("_padded")]
# a window that cuts something moves the store's base on the host: the store is needed before anything else is looked at
for e in DECODE_ATTN[1:]:
    HOST += [
        (e, dict(window=16, kv_start=None, k_store=None), E_NULL, "NULL store / scales / strides"),
        (e, dict(window=256, kv_start=None, v_st=None), E_NULL, "NULL store / scales / strides"),  # k_new given: lo = T + 1 - W = 1
    ]


@pytest.mark.parametrize("entry,over,rc,msg", _rows(HOST))
def test_refused_on_the_host(lib, entry, over, rc, msg):
    lib.kvq_kernel_log_clear()
    got, err = _call(lib, entry, **over)
    assert (got, err.startswith(_name(entry, over) + ": "), msg in err) == (rc, True, True), (got, err)
    assert lib.kvq_kernel_log(None, 0) == 0


def test_layers_entry_point_refuses_null_tables(lib):
    from efficient_llm_inference_amd._lib import KvqAttnDims, KvqStrides, byref
    st, dm = KvqStrides(0, 1 << 20, 1 << 17, 128), KvqAttnDims(1, 8, 8, 256, 128)
    tab = (ctypes.c_void_p * 1)(FAKE)
    ws = ctypes.c_void_p(FAKE)

    def layers(n=1, append=0, q=tab, k_new=tab, v_new=tab, k_store=tab, out=tab):
        return lib.kvq_decode_step_layers(n, append, q, 1024, 128, k_new, 1024, 128, v_new, 1024, 128, k_store, byref(st), tab, 8, tab,
                                          byref(st), tab, 8, out, 1024, 128, F16, 0.088, 1e-8, ws, BIG, byref(dm), None)

    for kw in (dict(n=-1), dict(q=None), dict(out=None), dict(k_store=None), dict(append=1, k_new=None, v_new=None), dict(v_new=None)):
        assert layers(**kw) == E_NULL, kw
        assert lib.kvq_last_error_string() == b"kvq_decode_step_layers: NULL pointer table (or n_layers < 0)", kw
    assert layers(n=0) == 0  # no layer: nothing to do


# (B, Hq, Hkv, T, D) -> kvq_decode_attn_workspace, kvq_decode_attn_workspace_cap
WORKSPACE = [
    ((1, 32, 8, 1000, 128), 33288, 37448),
    ((8, 32, 8, 16384, 128), 4259904, 4293184),
    ((3, 8, 2, 300, 32), 824, 1640),
    ((0, 8, 2, 300, 32), -1, -1),
    ((1, 8, 0, 300, 32), -1, -1),
    ((1, 8, 2, -1, 32), -1, -1),
    ((1, 8, 2, 300, 48), -1, -1),
    ((1, 8, 2, 300, 0), -1, -1),
]


@pytest.mark.parametrize("dims,floats,cap", WORKSPACE, ids=[",".join(map(str, w[0])) for w in WORKSPACE])
def test_workspace_sizes(lib, dims, floats, cap):
    from efficient_llm_inference_amd._lib import KvqAttnDims, byref
    d = KvqAttnDims(*dims)
    assert (lib.kvq_decode_attn_workspace(byref(d)), lib.kvq_decode_attn_workspace_cap(byref(d))) == (floats, cap)


def test_workspace_null_dims(lib):
    assert lib.kvq_decode_attn_workspace(None) == -1 and lib.kvq_decode_attn_workspace_cap(None) == -1
    assert lib.kvq_extend_attn_workspace(None) == -1


# ----------------------------------------------------------------------------------------------------------------- GPU rows
# The decode checks behind check_device(out). `big`: B * Hkv * D = 131072 elements of new token, past a device count's bound.
DEVICE = []
for e in DECODE_ATTN + DECODE_STEP + DECODE_STEP_DEV:
    dev = e in DECODE_STEP_DEV
    DEVICE += [
        (e, dict(dims=(1, 8, 3, 256, 128)), E_DIMS, "bad dims B=1 Hq=8 Hkv=3 T=256 (need Hq % Hkv == 0, Hq / Hkv <= 8, or <= 16 at head_dim 64 / 128)"),
        (e, dict(dims=(1, 34, 2, 256, 128)), E_DIMS, "bad dims B=1 Hq=34 Hkv=2 T=256"),
        (e, dict(dims=(1, 32, 2, 256, 32)), E_DIMS, "bad dims B=1 Hq=32 Hkv=2 T=256"),  # 16 per kv head only on the MFMA kernels
        (e, dict(dims=(1, 8, 8, 256, 48)), E_DIMS, "head_dim 48 not supported (32, 64, 128, 256)"),
        (e, dict(dtype=F32), E_DIMS if dev else E_DTYPE,
         "needs an upper bound T >= 1, B * Hkv * D <= 65536 and fp16 / bf16 tensors" if dev else "dtype 2 not supported (KVQ_F16, KVQ_BF16)"),
        (e, dict(k_bits=2), E_DIMS, "k_bits / v_bits must be 8 or 4"),
        (e, dict(v_bits=0), E_DIMS, "k_bits / v_bits must be 8 or 4"),
        (e, dict(ws_floats=8), E_DIMS, "workspace of 8 floats, 2088 needed"),
        (e, dict(k_store="off8"), E_DIMS, "store rows must be 16 / 16 byte aligned"),
        (e, dict(v_bits=4, v_st=(0, 1 << 20, 1 << 17, 68)), E_DIMS, "store rows must be 16 / 8 byte aligned"),
        (e, dict(q="off8"), E_DIMS, "q must be 16-byte aligned with strides that are multiples of 8 elements"),
        (e, dict(q_s=(1028, 128)), E_DIMS, "q must be 16-byte aligned with strides that are multiples of 8 elements"),
        (e, dict(ws="off8"), E_DIMS, "workspace must be 16-byte aligned"),
    ]
for e in DECODE_ATTN:
    DEVICE += [
        (e, dict(v_new=None), E_NULL, "k_new and v_new must be given together"),
        (e, dict(k_new=None), E_NULL, "k_new and v_new must be given together"),
        (e, dict(k_new=None, v_new=None, dims=(1, 8, 8, 0, 128)), E_DIMS, "nothing to attend to (T == 0 and no new token)"),
        (e, dict(k_scales=None), E_NULL, "NULL store / scales / strides / workspace"),
        (e, dict(ws=None), E_NULL, "NULL store / scales / strides / workspace"),
    ]
for e in DECODE_STEP_DEV:
    DEVICE += [
        (e, dict(dims=(16, 64, 64, 256, 128)), E_DIMS, "needs an upper bound T >= 1, B * Hkv * D <= 65536 and fp16 / bf16 tensors"),
        (e, dict(dims=(1, 8, 8, 0, 128)), E_DIMS, "needs an upper bound T >= 1, B * Hkv * D <= 65536 and fp16 / bf16 tensors"),
    ]


@pytest.fixture(scope="module")
def device_buffer():
    import torch
    return torch.zeros(64, dtype=torch.int32, device="cuda")  # every pointer of a GPU row: one real buffer, never touched


@pytest.mark.gpu
@pytest.mark.parametrize("entry,over,rc,msg", _rows(DEVICE))
def test_refused_behind_the_device_check(lib, device_buffer, entry, over, rc, msg):
    base = device_buffer.data_ptr()
    assert base % 16 == 0
    lib.kvq_kernel_log_clear()
    got, err = _call(lib, entry, base=base, **over)
    assert (got, err.startswith(entry + ": "), msg in err) == (rc, True, True), (got, err)
    assert lib.kvq_kernel_log(None, 0) == 0
    assert int(device_buffer.sum()) == 0
