"""The device side the ``gpu`` attention tests share: the two fixtures, a ``tests/attn_cases.Case`` put into device stores with
poison around it, the same case run through one of the four attention entry points, and the suite's standard tolerance check.
The float64 side is tests/attn_ref.py. Test modules import the fixtures by name:
``from tests.gpu_harness import K, tunable  # noqa: F401``."""
import numpy as np
import pytest
import torch

from tests.attn_cases import TOL, narrow, widen
from tests.util import NAME, TD, to_numpy, to_torch

POISON = {"nan": float("nan"), "huge": 1e30}  # fmaxf drops a NaN: a poisoned scale folded into a running max shows at 1e30 only
CASE = object()  # run_case: "what the case says"


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available()
    from efficient_llm_inference_amd import _lib, kernels
    _lib.load()
    return kernels


@pytest.fixture
def tunable():
    from efficient_llm_inference_amd import _lib
    touched = {}

    def set_(key, value):
        touched.setdefault(key, _lib.get_tunable(key))  # restore what the library shipped with, not 0
        _lib.set_tunable(key, value)
    yield set_
    for key, old in touched.items():
        _lib.set_tunable(key, old)


def dev_i32(values):
    return torch.tensor(list(values), dtype=torch.int32, device="cuda")


def got64(out, dtype=None):
    """a result tensor in the compute dtype -> float64 numpy"""
    return widen(to_numpy(out), dtype or NAME[out.dtype])


def rand_like(shape, dtype, rng, scale=1.0):
    """seeded Gaussian values in the compute dtype's numpy representation (fp16 array, bf16 as uint16 bits)"""
    return narrow((rng.standard_normal(shape) * scale).astype(np.float32), dtype)


def within_standard(got, ref, dtype, what=None):
    """The suite's standard tolerance on every element of ``got`` (float64 numpy, or a result tensor): finite and
    ``|got - ref| <= TOL * (|ref| + max |ref|)``."""
    got = got64(got) if torch.is_tensor(got) else np.asarray(got, np.float64)
    assert np.isfinite(got).all(), what
    err = np.abs(got - ref)
    lim = TOL[dtype] * (np.abs(ref) + np.abs(ref).max())
    assert (err <= lim).all(), (what, float(err.max()), float(np.abs(ref).max()), float((err / np.maximum(lim, 1e-30)).max()))


class DeviceStores:
    """What :func:`device_stores` returns: ``views`` = [K codes, K scales, V codes, V scales] of ``cap`` slots (also what
    iterating gives), inside ``bufs`` with ``guard`` more slots on each side."""

    def __init__(self, bufs, guard, cap):
        self.bufs, self.guard = bufs, guard
        self.views = [b[:, :, guard:guard + cap] if b.dim() == 4 else b[guard:guard + cap] for b in bufs]

    def __iter__(self):
        return iter(self.views)

    def slot(self, t):
        """slot t as numpy: (K row, V row, K scale, V scale)"""
        k, ks, v, vs = self.views
        return to_numpy(k[:, :, t]), to_numpy(v[:, :, t]), to_numpy(ks[t:t + 1]), to_numpy(vs[t:t + 1])


def device_stores(K, c, cap, poison, hide=None, guard=0):
    """Case ``c`` in device stores of ``cap`` slots. The slots that hold the case's codes and scales are filled with them;
    every other slot (the ``guard`` slots on each side, outside the views, included) holds extreme codes (127 / 0xFF) and the
    scale ``poison`` (NaN or 1e30). ``hide``: the first visible stored token, one for the batch (``c.lo``) or one per batch
    row (``c.los``): batch row b's codes below its own are extreme, and the scale slots below the smallest (the only ones no
    row needs) are poisoned."""
    T = c.T
    rows = [0] * c.B if hide is None else ([int(hide)] * c.B if np.ndim(hide) == 0 else [int(h) for h in hide])
    lo = min(rows)
    bufs = []
    for qa, sc, kind in ((c.kq, c.ks, c.kinds[0]), (c.vq, c.vs, c.kinds[1])):
        extreme = 127 if kind == "int8" else 0xFF
        codes = torch.full((c.B, c.Hkv, cap + 2 * guard, qa.shape[-1]), extreme, dtype=K.QDTYPE[kind], device="cuda")
        scales = torch.full((cap + 2 * guard,), poison, device="cuda")
        if T > lo:
            codes[:, :, guard + lo:guard + T] = to_torch(np.ascontiguousarray(qa[:, :, lo:]))
            scales[guard + lo:guard + T] = to_torch(np.ascontiguousarray(sc[lo:]))
            for b, h in enumerate(rows):
                codes[b, :, guard + lo:guard + h] = extreme
        bufs += [codes, scales]
    return DeviceStores(bufs, guard, cap)


def run_case(K, c, entry, window=CASE, kv_start=CASE, softcap=0.0, sinks=None, bound=None, cap=None, stores=None, kn=None,
             vn=None, place=None):
    """Case ``c`` through kernels.decode_attn ("attn"), decode_step ("step"), decode_step_dev ("dev": the count c.T in device
    memory under the host's ``bound``) or extend_attn ("extend"), with NaN in the output and the workspace beforehand.
    ``window`` / ``kv_start`` (a list): the case's own unless given; ``sinks``: numpy [Hq]; ``stores``: the
    :class:`DeviceStores` to run on (default: :func:`device_stores` of ``cap`` slots, T + 3 or bound + 8, with NaN scales);
    ``kn`` / ``vn``: new token(s) instead of the case's (numpy in the compute dtype's representation, or device tensors).
    ``place``: {"q" / "out" / "kn" / "vn": a device view of the tensor's shape and dtype}: the call's tensor is copied into
    the view and the view is what the library gets (strided and far layouts: tests/test_gpu_far_offsets.py).
    Returns (float64 result, kernel log, stores)."""
    from efficient_llm_inference_amd import _lib
    d = c.dtype
    assert (entry == "dev") == (bound is not None), (entry, bound)
    if stores is None:
        stores = device_stores(K, c, cap or (bound + 8 if bound else c.T + 3), POISON["nan"])
    k_store, k_sc, v_store, v_sc = stores
    starts = c.kv_start if kv_start is CASE else kv_start
    kw = dict(window=c.window if window is CASE else window, kv_start=None if starts is None else dev_i32(starts),
              softcap=softcap, sinks=None if sinks is None else to_torch(np.asarray(sinks, np.float32)))

    def new_token(x, own):
        x = own if x is None else x
        return x if (x is None or torch.is_tensor(x)) else to_torch(x, d)

    def put(name, x):
        if not place or name not in place or x is None:
            return x
        place[name].copy_(x)
        return place[name]
    kn, vn = put("kn", new_token(kn, c.kn)), put("vn", new_token(vn, c.vn))
    if entry == "extend":
        q = to_torch(c.q, d)
        n_ws = max(1, K.extend_attn_workspace(c.B, c.Hq, c.Hkv, c.T, c.S, c.D))
    else:
        q = to_torch(np.ascontiguousarray(c.q[:, :, 0]), d)
        n_ws = max(1, K.decode_attn_workspace_cap(c.B, c.Hq, c.Hkv, k_store.shape[2], c.D))
    q, out = put("q", q), put("out", torch.full(q.shape, float("nan"), dtype=TD[d], device="cuda"))
    ws = torch.full((n_ws,), float("nan"), device="cuda")
    _lib.kernel_log_clear()
    if entry == "extend":
        K.extend_attn(q, k_store, k_sc, c.kinds[0], v_store, v_sc, c.kinds[1], c.T, kn, vn, out, ws, c.sm, **kw)
    elif entry == "attn":
        K.decode_attn(q, k_store, k_sc, c.kinds[0], v_store, v_sc, c.kinds[1], c.T, out, ws, c.sm, kn, vn, **kw)
    else:
        plan = K.DecodeStepPlan(q, k_store, k_sc, c.kinds[0], v_store, v_sc, c.kinds[1], 1e-8)
        if entry == "step":
            K.decode_step(plan, q, kn, vn, c.T, out, ws, c.sm, **kw)
        else:
            K.decode_step_dev(plan, q, kn, vn, dev_i32([c.T]), bound, out, ws, c.sm, **kw)
    torch.cuda.synchronize()
    return got64(out, d), _lib.kernel_log(), stores
