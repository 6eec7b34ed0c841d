"""Left-padded batches (a per-row key start, ``kv_start``) in attention over the quantised store on the MI355X: host-count
decode (kvq_decode_attn_padded / kvq_decode_step_padded), device-count decode (kvq_decode_step_dev_padded, eager and
graph-replayed) and extend (kvq_extend_attn_padded) against the float64 model of tests/attn_ref.py, with the suite's own
tolerance (tests/gpu_harness.py::within_standard) on EVERY element: rows that see no key must be
exactly zero. Padding is never read (poisoned stores give the same bits), nothing existing moved (kv_start=None is the
windowed call), and every kernel family is seen in its padded form in the kernel log."""
import numpy as np
import pytest
import torch

from efficient_llm_inference_amd import _lib
from efficient_llm_inference_amd import kernels as K
from tests.attn_cases import BITS, dev_plan
from tests.attn_ref import decode as decode_ref
from tests.attn_ref import dequant
from tests.attn_ref import extend as extend_ref
from tests.gpu_harness import dev_i32, got64, within_standard
from tests.test_gpu_sliding_window import KINDS, SHAPES, Store, _inputs, _random_store
from tests.util import TD, tunables

pytestmark = pytest.mark.gpu

# the sliding-window file's shapes with the batch raised to 3 where it is 1 (per-row starts mean nothing at batch 1)
PSHAPES = [(max(B, 3), Hq, Hkv, D) for B, Hq, Hkv, D in SHAPES]


def _pick(xs):
    """every boundary when there are at most 8, else the first two, the middle one and the last two"""
    return xs if len(xs) <= 8 else xs[:2] + [xs[len(xs) // 2]] + xs[-2:]


def _patterns(B, T, plan, seed):
    """Start vectors [B] for a store of T tokens under ``plan`` (tests.attn_cases.dev_plan: the Python restatement of the
    host's split layout): all 0; all T; one row T, the rest 0; 63 .. 129 around the tile edges; both sides of the split
    boundaries; random. A padded row's splits start at ITS first visible token lo_b and cover lt = T - lo_b tokens, so two
    kinds of boundary are placed:
      * absolute: starts at k * ts - 1, k * ts, k * ts + 1 with ts the unpadded layout's tokens per split (the rows a start
        hides end next to a boundary of the layout the grid was planned for);
      * per row: starts at T - k * ts + 1, T - k * ts, T - k * ts - 1, so that the row's LIVE count lt sits on both sides of a
        multiple of its split size (one-tile routes: ts; the ring: nsplit * 64, where ring_dev_tpw's tiles per wave and with
        it the row's split size and live split count change).
    Every boundary when a layout has at most 8, else the first two, the middle and the last two (_pick): the float64
    reference, not the kernels, is what a case costs, and the suite is meant to stay about a minute."""
    ts = plan.live(T)[0]
    pats = [[0] * B, [T] * B, [T] + [0] * (B - 1)]
    vals = [63, 64, 65, 127, 128, 129]
    for k in _pick(list(range(ts, T, ts))):
        vals += [k - 1, k, k + 1]
    step = plan.nsplit * 64 if plan.tpw else plan.ts
    for k in _pick(list(range(step, T, step))):
        vals += [T - k + 1, T - k, T - k - 1]
    vals = [min(max(v, 0), T) for v in vals]
    for i in range(0, len(vals), B):
        pats.append([vals[(i + j) % len(vals)] for j in range(B)])
    rng = np.random.default_rng(seed)
    pats.append([int(x) for x in rng.integers(0, T + 1, B)])
    out = []
    for p in pats:
        if p not in out:
            out.append(p)
    return out


def _poisoned(clean, starts, T):
    """A copy of the store with row b's slots < starts[b] at the extreme codes, and NaN scales below min_b starts[b]
    (the only slots whose scale no row needs)."""
    st = clean.clone()
    for store, sc, kind in zip(st.q, st.s, clean.kinds):
        for b, s in enumerate(starts):
            store[b, :, :min(s, T)] = 127 if kind == "int8" else 0xFF
        sc[:min(min(starts), T)] = float("nan")
    return st


def _cases():
    out = []
    for si, shape in enumerate(PSHAPES):
        for ti, T in enumerate((0, 1, 63, 64, 65, 3100, 8200)):
            if T >= 3100 and (si >= 3 or (T == 8200 and si > 0)):
                continue
            kinds = KINDS[(si + ti) % 3] if not (shape[3] == 64 and shape[0] == 4) else ("int8", KINDS[ti % 3][1])
            out.append((shape, T, kinds, ("f16", "bf16")[(si + ti) % 2]))
    return out


@pytest.mark.parametrize("shape,T,kinds,dtype", _cases())
def test_host_count_decode_padded(shape, T, kinds, dtype):
    """kvq_decode_attn_padded with and without k_new against attn_ref, on a store whose padding is poisoned; the same bits
    on the clean store (padding is never read)."""
    B, Hq, Hkv, D = shape
    sm = D ** -0.5
    rng = np.random.default_rng(T + D)
    q, kn_t, vn_t, q_np, kn, vn = _inputs(rng, [(B, Hq, D), (B, Hkv, D), (B, Hkv, D)], dtype)
    clean = Store(B, Hkv, T, D, kinds, dtype, seed=T)
    ws = torch.empty(K.decode_attn_workspace_cap(B, Hq, Hkv, T + 2, D), dtype=torch.float32, device="cuda")
    pats = _patterns(B, T, dev_plan(B, Hq, Hkv, D, BITS[kinds[0]], max(T, 1), v_bits=BITS[kinds[1]]), seed=T)
    # The large stores (T >= 3100): every pattern runs, and for each of them every window; has_new alternates with the pattern
    # and the window (the float64 reference over 8 K tokens is what a combination costs). The small stores run everything.
    for pi, starts in enumerate(pats):
        for W in (0, 64, T + 1):
            for has_new in ((True, False) if T else (True,)):
                if T >= 3100 and (pi + (W > 0) + (W > 64) + has_new) % 2:
                    continue
                a = (kn_t, vn_t) if has_new else (None, None)
                ref = decode_ref(clean.deq[0], clean.deq[1], q_np, kn if has_new else None, vn, T, W, sm, starts)
                st = _poisoned(clean, starts, T)
                out = torch.full((B, Hq, D), float("nan"), dtype=TD[dtype], device="cuda")
                _lib.kernel_log_clear()
                K.decode_attn(q, st.q[0], st.s[0], kinds[0], st.q[1], st.s[1], kinds[1], T, out, ws, sm, *a, window=W,
                              kv_start=dev_i32(starts))
                torch.cuda.synchronize()
                log = _lib.kernel_log()
                assert log and all("_padded_k" in n for n in log), log
                within_standard(out, ref, dtype)
                o2 = torch.empty_like(out)
                K.decode_attn(q, clean.q[0], clean.s[0], kinds[0], clean.q[1], clean.s[1], kinds[1], T, o2, ws, sm, *a,
                              window=W, kv_start=dev_i32(starts))
                assert torch.equal(out, o2), (starts, W, has_new)
                if not has_new:  # rows that see no key: exactly zero
                    dead = [b for b, s in enumerate(starts) if s >= T]
                    assert all(bool((out[b] == 0).all()) for b in dead)
    # the step: the new token's slot T and scales[T] are what kvq_decode_step writes
    starts = pats[-1]
    a, b = _poisoned(clean, starts, T), clean.clone()
    pa = K.DecodeStepPlan(q, a.q[0], a.s[0], kinds[0], a.q[1], a.s[1], kinds[1], 1e-8)
    pb = K.DecodeStepPlan(q, b.q[0], b.s[0], kinds[0], b.q[1], b.s[1], kinds[1], 1e-8)
    oa, ob = torch.empty_like(q), torch.empty_like(q)
    K.decode_step(pa, q, kn_t, vn_t, T, oa, ws, sm, window=64, kv_start=dev_i32(starts))
    K.decode_step(pb, q, kn_t, vn_t, T, ob, ws, sm)
    torch.cuda.synchronize()
    within_standard(oa, decode_ref(clean.deq[0], clean.deq[1], q_np, kn, vn, T, 64, sm, starts), dtype)
    for i in range(2):
        assert torch.equal(a.q[i][:, :, T], b.q[i][:, :, T]) and torch.equal(a.s[i][T], b.s[i][T])


ROUTES = [  # name, shape, T, kinds, tunables, partial, merge
    ("VALU", (3, 8, 2, 32), 300, ("int4", "int4"), {}, "decode_attn_partial_padded_k<4, 4, 4>", "decode_attn_merge_fast_padded_k<2>"),
    ("VALU hd256", (3, 4, 1, 256), 700, ("int8", "int4"), {}, "decode_attn_partial_padded_k<8, 4, 4>", "decode_attn_merge_fast_padded_k<"),
    ("MFMA one wave", (3, 32, 8, 128), 1000, ("int8", "int4"), {}, "decode_attn_partial_mfma_padded_k<8, 4, 128, 128, false>",
     "decode_attn_merge_fast_padded_k<2>"),
    ("MFMA fast", (3, 32, 8, 128), 3100, ("int8", "int8"), {}, "decode_attn_partial_mfma_padded_k<8, 8, 128, 128, false>",
     "decode_attn_merge_fast_padded_k<16>"),
    ("MFMA hd64 chained", (4, 16, 4, 64), 900, ("int4", "int8"), {"attn_merge_fast": 0},
     "decode_attn_partial_mfma_padded_k<4, 8, 128, 64, false>", "decode_attn_merge_padded_k"),
    ("ring TG4", (4, 32, 8, 128), 8200, ("int8", "int4"), {}, "decode_attn_lds_mfma_padded_k<8, 4, 64, true, 2, 4, 128>",
     "decode_attn_merge_fast_padded_k<"),
    ("ring TG1", (4, 64, 8, 128), 1500, ("int4", "int4"), {"attn_stream_tpw": 3},
     "decode_attn_lds_mfma_padded_k<4, 4, 64, false, 2, 1, 128>", "decode_attn_merge_fast_padded_k<2>"),
    ("ring hd64 chained", (4, 32, 8, 64), 1500, ("int8", "int8"), {"attn_stream_tpw": 2, "attn_merge_fast": 0},
     "decode_attn_lds_mfma_padded_k<8, 8, 64, true, 2, 4, 64>", "decode_attn_merge_padded_k"),
]


@pytest.mark.parametrize("name,shape,T,kinds,tun,partial,merge", ROUTES, ids=[r[0] for r in ROUTES])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_every_route_in_its_padded_form(name, shape, T, kinds, tun, partial, merge, dtype):
    """Each kernel family (VALU, one-tile MFMA, ring; one-wave, fast and chained merge) is launched in its padded form, host
    count and device count, and matches attn_ref with starts on both sides of the route's split boundaries and a window
    that wins for some rows while the start wins for others."""
    B, Hq, Hkv, D = shape
    sm = D ** -0.5
    rng = np.random.default_rng(T)
    q, kn_t, vn_t, q_np, kn, vn = _inputs(rng, [(B, Hq, D), (B, Hkv, D), (B, Hkv, D)], dtype)
    clean = Store(B, Hkv, T, D, kinds, dtype, seed=T)
    bound = T + 40
    ws = torch.empty(K.decode_attn_workspace_cap(B, Hq, Hkv, bound + 2, D), dtype=torch.float32, device="cuda")
    with tunables(**tun):
        plan = dev_plan(B, Hq, Hkv, D, BITS[kinds[0]], T, tunables=tun, v_bits=BITS[kinds[1]])
        for starts in _patterns(B, T, plan, seed=T)[2:]:
            for W in (0, T // 2):
                dstarts = dev_i32(starts)
                st = _poisoned(clean, starts, T)
                ref = decode_ref(clean.deq[0], clean.deq[1], q_np, kn, vn, T, W, sm, starts)
                out = torch.full((B, Hq, D), float("nan"), dtype=TD[dtype], device="cuda")
                _lib.kernel_log_clear()
                K.decode_attn(q, st.q[0], st.s[0], kinds[0], st.q[1], st.s[1], kinds[1], T, out, ws, sm, kn_t, vn_t, window=W,
                              kv_start=dstarts)
                torch.cuda.synchronize()
                log = _lib.kernel_log()
                if W == 0:  # the planned route (a window plans for fewer tokens and may take another)
                    assert log[0] == partial and log[1].startswith(merge), (name, log)
                assert all("_padded_k" in n for n in log), log
                within_standard(out, ref, dtype)
                # device count: the store has spare slots; the count equals T
                pl = K.DecodeStepPlan(q, st.q[0], st.s[0], kinds[0], st.q[1], st.s[1], kinds[1], 1e-8)
                od = torch.full_like(out, float("nan"))
                _lib.kernel_log_clear()
                K.decode_step_dev(pl, q, kn_t, vn_t, dev_i32([T]), T + 3, od, ws, sm, window=W, kv_start=dstarts)
                torch.cuda.synchronize()
                assert all("_padded_k" in n for n in _lib.kernel_log()), _lib.kernel_log()
                within_standard(od, ref, dtype)


@pytest.mark.parametrize("shape,kinds,W,tun", [((16, 32, 8, 128), ("int8", "int4"), 0, {}),
                                               ((16, 32, 8, 128), ("int8", "int8"), 2000, {"attn_merge_fast": 0}),
                                               ((3, 32, 8, 128), ("int8", "int4"), 200, {}),
                                               ((4, 32, 8, 64), ("int8", "int8"), 130, {}),
                                               ((3, 8, 2, 32), ("int4", "int4"), 40, {})])
def test_device_count_decode_padded(shape, kinds, W, tun):
    """kvq_decode_step_dev_padded (eager) at counts below, at and above some rows' starts, count 0 included, against
    attn_ref; the stores it leaves are those of the unpadded device-count step."""
    B, Hq, Hkv, D = shape
    dtype, sm, bound = "f16", D ** -0.5, 2100
    rng = np.random.default_rng(W + B)
    q, kn_t, vn_t, q_np, kn, vn = _inputs(rng, [(B, Hq, D), (B, Hkv, D), (B, Hkv, D)], dtype)
    clean = Store(B, Hkv, bound, D, kinds, dtype, seed=W, cap=bound + 2)
    ws = torch.empty(K.decode_attn_workspace_cap(B, Hq, Hkv, bound + 1, D), dtype=torch.float32, device="cuda")
    starts = [int(x) for x in np.random.default_rng(B).integers(0, 1400, B)]
    starts[0], starts[1], starts[2] = 0, 1000, 64
    seen = set()
    with tunables(**tun):
        for t in (0, 1, 63, 64, 65, 999, 1000, 1001, 2047, 2049, bound):
            a = _poisoned(clean, [min(s, t) for s in starts], t)
            b = clean.clone()
            pa = K.DecodeStepPlan(q, a.q[0], a.s[0], kinds[0], a.q[1], a.s[1], kinds[1], 1e-8)
            pb = K.DecodeStepPlan(q, b.q[0], b.s[0], kinds[0], b.q[1], b.s[1], kinds[1], 1e-8)
            oa, ob = torch.full_like(q, float("nan")), torch.empty_like(q)
            t_dev = dev_i32([t])
            _lib.kernel_log_clear()
            K.decode_step_dev(pa, q, kn_t, vn_t, t_dev, bound, oa, ws, sm, window=W, kv_start=dev_i32(starts))
            seen |= set(_lib.kernel_log())
            K.decode_step_dev(pb, q, kn_t, vn_t, t_dev, bound, ob, ws, sm, window=W)
            torch.cuda.synchronize()
            within_standard(oa, decode_ref(clean.deq[0], clean.deq[1], q_np, kn, vn, t, W, sm, starts), dtype)
            for i in range(2):
                assert torch.equal(a.q[i][:, :, t], b.q[i][:, :, t]) and torch.equal(a.s[i][t], b.s[i][t]), t
    assert all("_padded_k" in n for n in seen), seen
    if B == 16:  # the ring kernel under a count
        assert any(n.startswith("decode_attn_lds_mfma_padded_k<") for n in seen), seen


EXT = [  # B, Hq, Hkv, T, D, kinds, dtype
    (3, 8, 8, 300, 128, ("int8", "int4"), "f16"),
    (3, 32, 8, 1000, 128, ("int8", "int8"), "bf16"),
    (3, 8, 2, 0, 64, ("int4", "int4"), "f16"),
    (3, 16, 4, 4000, 64, ("int4", "int8"), "f16"),
]


@pytest.mark.parametrize("B,Hq,Hkv,T,D,kinds,dtype", EXT)
@pytest.mark.parametrize("S", [1, 40, 130])
def test_extend_padded(B, Hq, Hkv, T, D, kinds, dtype, S):
    """kvq_extend_attn_padded: starts in the store, at T, and reaching into the chunk (rows whose own position is padding are
    zeros), crossed with windows; the stored padding AND the chunk's padded prefix are poisoned and never read."""
    sm = D ** -0.5
    rng = np.random.default_rng(T + S)
    q, knt, vnt, q_np, kn, vn = _inputs(rng, [(B, Hq, S, D), (B, Hkv, S, D), (B, Hkv, S, D)], dtype)
    clean = Store(B, Hkv, T, D, kinds, dtype, seed=T)
    ws = torch.full((max(1, K.extend_attn_workspace(B, Hq, Hkv, T, S, D)),), float("nan"), device="cuda")
    pats = [[0] * B, [T] * B, [T + S - 1, 0, T // 2], [min(63, T), T + S // 2, min(65, T)], [T + S, 129, T + 1][:B],
            [int(x) for x in rng.integers(0, T + S + 1, B)]]
    dt = {"f16": 0, "bf16": 1}[dtype]
    for starts in pats:
        for W in (0, 64, T + 1):
            ref = extend_ref(clean.deq[0], clean.deq[1], q_np, kn, vn, T, W, sm, starts)
            st = _poisoned(clean, starts, T)
            kp, vp = knt.clone(), vnt.clone()
            for b, s in enumerate(starts):  # the chunk's padded prefix
                if s > T:
                    kp[b, :, :s - T] = float("nan")
                    vp[b, :, :s - T] = float("inf")
            out = torch.full((B, Hq, S, D), float("nan"), dtype=TD[dtype], device="cuda")
            _lib.kernel_log_clear()
            K.extend_attn(q, st.q[0], st.s[0], kinds[0], st.q[1], st.s[1], kinds[1], T, kp, vp, out, ws, sm, window=W,
                          kv_start=dev_i32(starts))
            torch.cuda.synchronize()
            log = _lib.kernel_log()
            assert log[0] == f"extend_attn_padded_k<{BITS[kinds[0]]}, {BITS[kinds[1]]}, {D}, {dt}>" and \
                log[1:] in ([], [f"extend_attn_merge_padded_k<{D}, {dt}>"]), log
            within_standard(out, ref, dtype)
            o2 = torch.empty_like(out)
            K.extend_attn(q, clean.q[0], clean.s[0], kinds[0], clean.q[1], clean.s[1], kinds[1], T, knt, vnt, o2, ws, sm,
                          window=W, kv_start=dev_i32(starts))
            assert torch.equal(out, o2), (starts, W)
            for b, s in enumerate(starts):  # rows whose own position is padding: exactly zero
                if s > T:
                    assert bool((out[b, :, :min(s - T, S)] == 0).all()), (starts, W)


def test_nothing_existing_moved():
    """kv_start == NULL in each of the four padded entry points, called through ctypes, is the windowed call: the same kernel
    log, the same output bits and (the two steps) the same store bytes; all-zero starts on the device-count route equal
    kvq_decode_step_dev_window at the same count bit for bit."""
    B, Hq, Hkv, T, D, S = 3, 32, 8, 700, 128, 40
    kinds, sm = ("int8", "int4"), 128 ** -0.5
    rng = np.random.default_rng(5)
    q, kn, vn = _inputs(rng, [(B, Hq, D), (B, Hkv, D), (B, Hkv, D)], "f16")[:3]
    qe, kne, vne = _inputs(rng, [(B, Hq, S, D), (B, Hkv, S, D), (B, Hkv, S, D)], "f16")[:3]
    base = Store(B, Hkv, T, D, kinds, "f16", seed=2)
    ws = torch.empty(K.decode_attn_workspace_cap(B, Hq, Hkv, T + 8, D), dtype=torch.float32, device="cuda")
    wse = torch.empty(max(1, K.extend_attn_workspace(B, Hq, Hkv, T, S, D)), device="cuda")
    t_dev = dev_i32([T])
    lib = _lib.load()
    P = _lib.c_void_p
    stream = _lib.current_stream(q.device)

    def call(name, padded, W):
        """one entry point on a fresh copy of the store: (kernel log, output, store)"""
        st = base.clone()
        kst = _lib.KvqStrides(0, st.q[0].stride(0), st.q[0].stride(1), st.q[0].stride(2))
        vst = _lib.KvqStrides(0, st.q[1].stride(0), st.q[1].stride(1), st.q[1].stride(2))
        stores = [P(st.q[0].data_ptr()), _lib.byref(kst), P(st.s[0].data_ptr()), 8,
                  P(st.q[1].data_ptr()), _lib.byref(vst), P(st.s[1].data_ptr()), 4]
        win = [W, None] if padded else [W]
        dims = _lib.byref(_lib.KvqAttnDims(B, Hq, Hkv, T, D))
        if name == "extend_attn":
            o = torch.empty_like(qe)
            args = [P(qe.data_ptr()), *qe.stride()[:3], *stores, P(kne.data_ptr()), *kne.stride()[:3], P(vne.data_ptr()),
                    *vne.stride()[:3], P(o.data_ptr()), *o.stride()[:3], 0, sm, *win, P(wse.data_ptr()), wse.numel(),
                    _lib.byref(_lib.KvqExtendDims(B, Hq, Hkv, T, S, D)), stream]
        else:
            o = torch.empty_like(q)
            new = [P(kn.data_ptr()), kn.stride(0), kn.stride(1), P(vn.data_ptr()), vn.stride(0), vn.stride(1)]
            qa, oa = [P(q.data_ptr()), q.stride(0), q.stride(1)], [P(o.data_ptr()), o.stride(0), o.stride(1), 0, sm]
            wsa = [P(ws.data_ptr()), ws.numel(), dims]
            if name == "decode_attn":
                args = [*qa, *stores, *new, *oa, *win, *wsa, stream]
            elif name == "decode_step":
                args = [*qa, *new, *stores, *oa, *win, 1e-8, *wsa, stream]
            else:  # decode_step_dev: dims->T is the bound, the count is T
                wsa[2] = _lib.byref(_lib.KvqAttnDims(B, Hq, Hkv, T + 3, D))
                args = [*qa, *new, *stores, *oa, *win, 1e-8, *wsa, P(t_dev.data_ptr()), stream]
        fn = getattr(lib, f"kvq_{name}_{'padded' if padded else 'window'}")
        _lib.kernel_log_clear()
        rc = fn(*args)
        assert rc == 0, (name, padded, lib.kvq_last_error_string())
        torch.cuda.synchronize()
        return _lib.kernel_log(), o, st

    for name in ("decode_attn", "decode_step", "decode_step_dev", "extend_attn"):
        for W in (0, 64, 300):
            (log_w, out_w, st_w), (log_p, out_p, st_p) = call(name, False, W), call(name, True, W)
            assert log_w == log_p and not any("_padded_k" in n for n in log_p), (name, W, log_w, log_p)
            assert torch.equal(out_w, out_p), (name, W)
            for i in range(2):
                assert torch.equal(st_w.q[i], st_p.q[i]) and torch.equal(st_w.s[i], st_p.s[i]), (name, W)
    for shape in ((3, 32, 8, 128), (16, 32, 8, 128), (3, 8, 2, 32)):
        B, Hq, Hkv, D = shape
        bound, t = 2100, 1650
        q, kn, vn = _inputs(np.random.default_rng(D), [(B, Hq, D), (B, Hkv, D), (B, Hkv, D)], "f16")[:3]
        base = _random_store(B, Hkv, bound + 2, D, kinds, seed=D)
        ws = torch.empty(K.decode_attn_workspace_cap(B, Hq, Hkv, bound + 1, D), dtype=torch.float32, device="cuda")
        for W in (0, 512):
            outs = []
            for ks in (None, torch.zeros(B, dtype=torch.int32, device="cuda")):
                s2 = base.clone()
                plan = K.DecodeStepPlan(q, s2.q[0], s2.s[0], kinds[0], s2.q[1], s2.s[1], kinds[1], 1e-8)
                o = torch.empty_like(q)
                K.decode_step_dev(plan, q, kn, vn, dev_i32([t]), bound, o, ws, D ** -0.5, window=W, kv_start=ks)
                torch.cuda.synchronize()
                outs.append((o, s2))
            assert torch.equal(outs[0][0], outs[1][0]), (shape, W)
            for i in range(2):
                assert torch.equal(outs[0][1].q[i], outs[1][1].q[i]) and torch.equal(outs[0][1].s[i], outs[1][1].s[i])


def test_device_count_padded_graph_replay():
    """One captured kvq_decode_step_dev_padded step with a window, replayed while the count passes a tile boundary and the
    window's bound overtakes the smallest start: every step matches attn_ref. One capture, plain replay."""
    B, Hq, Hkv, D, W, T0, n = 3, 32, 8, 128, 48, 110, 40
    kinds, dtype, sm, bound = ("int8", "int4"), "f16", D ** -0.5, 256
    starts = [70, 0, 120]  # the window's bound T + 1 - 48 passes 70 at T = 117; T passes the tile edge 128
    clean = Store(B, Hkv, T0, D, kinds, dtype, seed=9, cap=bound + 2)
    st = _poisoned(clean, starts, T0)
    kd, vd = clean.deq[0].copy(), clean.deq[1].copy()
    g = torch.Generator(device="cuda").manual_seed(3)
    q = torch.empty(B, Hq, D, dtype=torch.float16, device="cuda")
    kn = torch.empty(B, Hkv, D, dtype=torch.float16, device="cuda")
    vn = torch.empty_like(kn)
    out = torch.empty_like(q)
    ws = torch.empty(K.decode_attn_workspace_cap(B, Hq, Hkv, bound + 1, D), dtype=torch.float32, device="cuda")
    t_dev = dev_i32([T0])
    ks = dev_i32(starts)
    plan = K.DecodeStepPlan(q, st.q[0], st.s[0], kinds[0], st.q[1], st.s[1], kinds[1], 1e-8)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture, on a scratch copy
        c = st.clone()
        pc = K.DecodeStepPlan(q, c.q[0], c.s[0], kinds[0], c.q[1], c.s[1], kinds[1], 1e-8)
        q.normal_(generator=g), kn.normal_(generator=g), vn.normal_(generator=g)
        K.decode_step_dev(pc, q, kn, vn, t_dev, bound, out, ws, sm, window=W, kv_start=ks)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        K.decode_step_dev(plan, q, kn, vn, t_dev, bound, out, ws, sm, window=W, kv_start=ks)
        t_dev.add_(1)
    for step in range(n):
        T = T0 + step
        q.copy_(torch.randn(B, Hq, D, generator=g, device="cuda"))
        kn.copy_(torch.randn(B, Hkv, D, generator=g, device="cuda"))
        vn.copy_(torch.randn(B, Hkv, D, generator=g, device="cuda"))
        graph.replay()
        torch.cuda.synchronize()
        within_standard(out, decode_ref(kd, vd, got64(q), got64(kn), got64(vn), T, W, sm, starts), dtype)
        # the token the step stored, as the store holds it
        kd = np.concatenate([kd[:, :, :T], dequant(st.q[0][:, :, T:T + 1].cpu().numpy(), st.s[0][T:T + 1].cpu().numpy(), kinds[0], D)], axis=2)
        vd = np.concatenate([vd[:, :, :T], dequant(st.q[1][:, :, T:T + 1].cpu().numpy(), st.s[1][T:T + 1].cpu().numpy(), kinds[1], D)], axis=2)
    assert int(t_dev.item()) == T0 + n


@pytest.mark.parametrize("arch", ["mistral-mini", "llama-mini"])
def test_fused_left_padded_batch_tracks_tuple_path(arch):
    """HF level: batch 3 with left padding of 0, 7 and about 40 % of a ~100-token prompt. The fused logits of every row's
    last position track the tuple path run on the SAME padded batch (relative max error < 2e-2, the bound of
    test_fused_sliding_window_model_tracks_tuple_path) over the prompt, 48 teacher-forced decode steps and a 16-token second
    turn through the padded extend; layer 0's store and scales are the tuple path's bit for bit; nothing non-finite is
    stored. (Graph-mode decode: test_fused_left_padded_graph_decode_emits_the_eager_tokens.)"""
    import efficient_llm_inference_amd as E
    from efficient_llm_inference_amd.benchmarking import from_legacy_tuple, to_legacy_tuple
    from efficient_llm_inference_amd.benchmarking.offline import load_model
    from efficient_llm_inference_amd.quantization import fused_attention as FA
    from transformers.cache_utils import DynamicCache
    model, tok = load_model(arch, "cuda", torch.float16)
    n_new, n_turn, B = 48, 16, 3
    with torch.no_grad():
        base = tok("<100>", return_tensors="pt").input_ids.cuda()
        P = base.shape[-1]
        g = torch.Generator(device="cuda").manual_seed(11)
        ids = torch.randint(1, 200, (B, P), generator=g, device="cuda")
        ids[0] = base[0]
        turn = torch.randint(1, 200, (B, n_turn), generator=g, device="cuda")
        pads = [0, 7, (P * 2) // 5]
        mask = torch.ones(B, P, dtype=torch.long, device="cuda")
        for b, n in enumerate(pads):
            mask[b, :n] = 0

        def grown(n):
            return torch.cat([mask, torch.ones(B, n, dtype=torch.long, device="cuda")], dim=1)

        out = model(input_ids=ids, attention_mask=mask, use_cache=True, past_key_values=DynamicCache())
        logits = out.logits[:, -1, :]
        kv = to_legacy_tuple(out.past_key_values)
        assert all(bool(torch.isfinite(k).all()) and bool(torch.isfinite(v).all()) for k, v in kv)
        qc = E.QuantizedKVCache(len(kv), "mixed", incremental=False)
        qc.init_from_prompt_past(kv)
        first = logits.float()
        ref_logits, toks = [], []
        for step in range(n_new):
            nxt = torch.argmax(logits, dim=-1, keepdim=True)
            toks.append(nxt)
            out = model(input_ids=nxt, attention_mask=grown(step + 1), use_cache=True,
                        past_key_values=from_legacy_tuple(qc.to_past_key_values()))
            logits = out.logits[:, -1, :]
            qc.append_from_past(to_legacy_tuple(out.past_key_values))
            ref_logits.append(logits.float())
        out = model(input_ids=turn, attention_mask=grown(n_new + n_turn), use_cache=True,
                    past_key_values=from_legacy_tuple(qc.to_past_key_values()))
        ref_turn = out.logits[:, -1, :].float()

        fc = FA.FusedQuantizedCache(len(kv), mode="mixed", reserve=P + n_new + n_turn)
        assert fc.set_left_padding(mask).tolist() == pads
        _lib.kernel_log_clear()
        with FA.fused_attention(model, fc) as cache:
            out = model(input_ids=ids, attention_mask=mask, use_cache=True, past_key_values=cache)
            got = out.logits[:, -1, :].float()
            assert float((got - first).abs().max() / first.abs().max()) < 2e-2
            worst = 0.0
            for step, nxt in enumerate(toks):
                got = model(input_ids=nxt, attention_mask=grown(step + 1), use_cache=True,
                            past_key_values=cache).logits[:, -1, :].float()
                assert torch.isfinite(got).all(), step
                worst = max(worst, float((got - ref_logits[step]).abs().max() / ref_logits[step].abs().max()))
            print("left-padded", arch, "worst relative logit error over decode", worst)
            assert worst < 2e-2, worst
            got = model(input_ids=turn, attention_mask=grown(n_new + n_turn), use_cache=True,
                        past_key_values=cache).logits[:, -1, :].float()
            err = float((got - ref_turn).abs().max() / ref_turn.abs().max())
            print("left-padded", arch, "second turn relative logit error", err)
            assert err < 2e-2, err
        log = _lib.kernel_log()
        assert any("decode_attn" in n and "_padded_k" in n for n in log) and any(n.startswith("extend_attn_padded_k<") for n in log), log
        T = P + n_new
        assert torch.isfinite(fc.qcache._k.scales[:, :T + n_turn]).all() and torch.isfinite(fc.qcache._v.scales[:, :T + n_turn]).all()
        assert torch.equal(fc.qcache._k.q[0, :, :, :T], qc._k.q[0, :, :, :T])
        assert torch.equal(fc.qcache._v.q[0, :, :, :T], qc._v.q[0, :, :, :T])
        assert torch.equal(fc.qcache._k.scales[0, :T], qc._k.scales[0, :T])
        assert torch.equal(fc.qcache._v.scales[0, :T], qc._v.scales[0, :T])


@pytest.mark.parametrize("arch", ["mistral-mini", "llama-mini"])
def test_fused_left_padded_graph_decode_emits_the_eager_tokens(arch):
    """HF level, graph mode: the left-padded batch of 3 decoded greedily by the eager fused path, then again with the decode
    step captured ONCE (kvq_decode_step_dev_padded per layer under ``t_dev``; static input ids, position ids and the static
    full-length attention mask passed to the model inside the capture; two warm-up steps on a side stream) and replayed:
    the replayed tokens are the eager ones, and the stores the two runs leave are equal. One capture, plain replay."""
    from efficient_llm_inference_amd.benchmarking.offline import load_model
    from efficient_llm_inference_amd.quantization import fused_attention as FA
    model, tok = load_model(arch, "cuda", torch.float16)
    n_steps, B = 40, 3  # mistral-mini: the 64-token window's bound overtakes the padded rows' starts on the way
    with torch.no_grad():
        P = tok("<100>", return_tensors="pt").input_ids.shape[-1]
        g = torch.Generator(device="cuda").manual_seed(11)
        ids = torch.randint(1, 200, (B, P), generator=g, device="cuda")
        pads = [0, 7, (P * 2) // 5]
        full = torch.ones(B, P + n_steps, dtype=torch.long, device="cuda")  # the static full-length mask
        for b, n in enumerate(pads):
            full[b, :n] = 0
        mask = full[:, :P].contiguous()
        n_layers = model.config.num_hidden_layers

        # eager fused decode
        fe = FA.FusedQuantizedCache(n_layers, mode="mixed", reserve=P + n_steps)
        fe.set_left_padding(mask)
        eager = []
        with FA.fused_attention(model, fe) as cache:
            logits = model(input_ids=ids, attention_mask=mask, use_cache=True, past_key_values=cache).logits[:, -1, :]
            for step in range(n_steps):
                nxt = torch.argmax(logits, dim=-1, keepdim=True)
                eager.append(nxt)
                logits = model(input_ids=nxt, attention_mask=full[:, :P + step + 1], use_cache=True,
                               past_key_values=cache).logits[:, -1, :]
        eager = torch.cat(eager, dim=1)

        # graph mode: the same steps, captured once
        fc = FA.FusedQuantizedCache(n_layers, mode="mixed", reserve=P + n_steps)
        fc.set_left_padding(mask)
        qc = fc.qcache
        _lib.kernel_log_clear()
        with FA.fused_attention(model, fc) as cache:
            logits = model(input_ids=ids, attention_mask=mask, use_cache=True, past_key_values=cache).logits[:, -1, :]
            T0 = qc._k.lens[0]
            assert T0 == P
            static_ids = torch.argmax(logits, dim=-1, keepdim=True).clone()
            gen = torch.zeros(B, n_steps, dtype=static_ids.dtype, device="cuda")
            pos = torch.full((B, 1), T0, dtype=torch.long, device="cuda")
            step_i = torch.zeros(1, dtype=torch.long, device="cuda")
            fc.t_dev = torch.full((1,), T0, dtype=torch.int32, device="cuda")
            fc.t_bound = T0 + n_steps - 1

            def body():
                gen.index_copy_(1, step_i, static_ids)
                out = model(input_ids=static_ids, attention_mask=full, position_ids=pos, use_cache=True, past_key_values=cache)
                static_ids.copy_(torch.argmax(out.logits[:, -1, :], dim=-1, keepdim=True))
                pos.add_(1)
                step_i.add_(1)
                fc.t_dev.add_(1)

            try:
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    body()
                    body()
                torch.cuda.current_stream().wait_stream(side)
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    body()
                for _ in range(n_steps - 2):
                    graph.replay()
                torch.cuda.synchronize()
            finally:
                fc.t_dev = None
        log = _lib.kernel_log()
        assert any("decode_attn" in n and "_padded_k" in n for n in log), log
        assert int(step_i.item()) == n_steps
        assert torch.equal(gen, eager), (gen != eager).nonzero()[:5]
        T = P + n_steps
        for a, b in ((fc.qcache._k, fe.qcache._k), (fc.qcache._v, fe.qcache._v)):
            assert torch.equal(a.q[:, :, :, :T], b.q[:, :, :, :T]) and torch.equal(a.scales[:, :T], b.scales[:, :T])
