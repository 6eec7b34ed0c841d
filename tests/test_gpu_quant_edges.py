"""Every quantise and dequantise route against the oracle on the edge families of tests/quant_cases.py, bit for bit.

Quantise: each row of test_gpu_quant_routing.ROWS that stores (kvq_quant_i8/i4_tokens and the from_absmax entry point,
on every kernel family it can route to) runs the exhaustive-value, tie, position-probe and eps families; the
from_absmax rows also run caller-given tables, including tables below the data (the clamp) and zeros (the eps floor).
The store is a window with a guard token on each side and the scale table a window with a guard column on each side:
both guards must come back untouched. The kernel log must be the row's, so the data cannot move a call to another route.
Each route gets one tensor of its row's shape per case: the larger rows (tile128, wide, split, chunk_fallback, ...) see
every finite value of the exhaustive family, the small ones (generic_odd_d, from_vec, wave_ragged, ...) a strided subset
of it; test_quant_discrimination.py covers the whole sets on the CPU.

Non-finite inputs (quant_cases.nonfinite_cases: NaN, +inf, -inf and their mixes in some tokens, caller-given tables over
them, NaN / +inf table entries) go through the same rows, the abs-max rows, the appends and the store's dequantise, with
the family's comparison rule: codes bit for bit, and for scale words and float outputs any NaN where the oracle has a
NaN, the oracle's bits everywhere else.

Appends that quantise with code of their own: the decode step's new token (merge.inc's register, parts and block
routines, through kvq_decode_step and kvq_decode_step_dev), QuantizedKVCache.extend's chunk and the sharded joint K + V
append on one rank, each with every family including the eps cases.

Dequantise: all 256 INT8 codes / packed INT4 bytes against scales with subnormal, overflowing, tie and +-0 products,
through the token kernels (fast and generic) for every output dtype and the flat fp16 entry points (chunk, vector and
scalar kernels)."""
import numpy as np
import pytest
import torch

from oracle import kvq_oracle as O
from tests import quant_cases as C
from tests.test_gpu_quant_routing import BF16, F16, F32, ROWS, TORCH, tile
from tests.util import bits, to_numpy, to_torch, tunables

pytestmark = pytest.mark.gpu

DT = {F16: "f16", BF16: "bf16", F32: "f32"}
QROWS = [r for r in ROWS if r[1] in ("i8", "i4", "from8", "from4") and r[8] == 0]
GUARD_Q, GUARD_S = 0xA5, -7.25


def _place(layout, x_cpu):
    """the row's input layout around the case's data (what test_gpu_quant_routing._input builds around random data)"""
    G = x_cpu.shape[0]
    if layout == "contig":
        return x_cpu.cuda()
    if layout == "bstride":
        full = torch.zeros((G, 2 * x_cpu.shape[1]) + tuple(x_cpu.shape[2:]), dtype=x_cpu.dtype)
        full[:, ::2] = x_cpu
        full[:, 1::2] = 1e4  # the skipped rows would raise every abs-max if a kernel read them
        return full.cuda()[:, ::2]
    xs = [x_cpu[g].cuda() for g in range(G - 1)]
    n = x_cpu[0].numel()
    buf = torch.empty(n + 8, dtype=x_cpu.dtype, device="cuda")
    last = buf[1:1 + n].view(x_cpu.shape[1:])
    last.copy_(x_cpu[G - 1])
    assert last.data_ptr() % 16 != 0
    return xs + [last]


def _launch(entry, x, ws, table, q, scales, eps):
    from efficient_llm_inference_amd import _lib, kernels
    from efficient_llm_inference_amd._lib import byref, c_void_p
    base, arr, ist, (G, B, H, T, D), dt, dev, _keep = kernels._in_views(x)
    lib, dims, dcode = _lib.load(), _lib.dims5(G, B, H, T, D), _lib.dtype_code(dt)
    wsp = c_void_p(ws.data_ptr()) if ws is not None else None
    if entry in ("i8", "i4"):
        fn = lib.kvq_quant_i8_tokens if entry == "i8" else lib.kvq_quant_i4_tokens
        return kernels._launch(dev, fn, base, arr, byref(ist), dcode, c_void_p(q.data_ptr()), byref(_lib.strides4(q)),
                               c_void_p(scales.data_ptr()), scales.stride(0), wsp, float(eps), byref(dims))
    return kernels._launch(dev, lib.kvq_quant_tokens_from_absmax, 8 if entry == "from8" else 4, base, arr, byref(ist), dcode,
                           c_void_p(q.data_ptr()), byref(_lib.strides4(q)), c_void_p(scales.data_ptr()), scales.stride(0),
                           c_void_p(table.data_ptr()), float(eps), byref(dims))


def _check_row(row, cases):
    """Every case through the row's entry point into a guarded store window: codes bit for bit, scale words by
    quant_cases.float_mismatch (plain bit equality wherever the oracle's scale is no NaN: every finite family)."""
    from efficient_llm_inference_amd import _lib, kernels
    name, entry, dtype, dims, layout, knobs, with_ws, want, _rc, _check = row
    G, B, H, T, D = dims
    kind = "int4" if entry in ("i4", "from4") else "int8"
    given = entry.startswith("from")
    Dq = kernels.packed_dim(kind, D)
    store = torch.empty(G, B, H, T + 2, Dq, dtype=kernels.QDTYPE[kind], device="cuda")
    sc = torch.empty(G, T + 2, dtype=torch.float32, device="cuda")
    failures = []
    for case in cases(dims, DT[dtype], kind, given):
        x = _place(layout, to_torch(case.x, DT[dtype], device="cpu").view(TORCH[dtype]))
        table = case.table if case.table is not None else C.data_absmax(case.x, case.dtype)
        store.view(torch.uint8).fill_(GUARD_Q)
        sc.fill_(GUARD_S)
        q, scales = store[:, :, :, 1:T + 1], sc[:, 1:T + 1]
        ws = torch.full((G * T,), -1.0, dtype=torch.float32, device="cuda") if with_ws else None
        tab = torch.from_numpy(np.ascontiguousarray(table, dtype=np.float32)).cuda()
        with tunables(**knobs):
            _lib.kernel_log_clear()
            rc = _launch(entry, x, ws, tab, q, scales, case.eps)
            torch.cuda.synchronize()
            log = _lib.kernel_log()
        assert rc == 0, (case.name, _lib.load().kvq_last_error_string())
        assert log == want, (case.name, log)
        q_ref, s_ref = C.reference(case, kind)
        got = to_numpy(store)
        if not np.array_equal(got[:, :, :, 1:T + 1], q_ref):
            bad = np.argwhere(got[:, :, :, 1:T + 1] != q_ref)
            failures.append(f"{case.name}: {len(bad)} store bytes differ, first at {tuple(bad[0])}: "
                            f"{got[:, :, :, 1:T + 1][tuple(bad[0])]} vs {q_ref[tuple(bad[0])]}")
        bad_s = C.float_mismatch(to_numpy(scales), s_ref, "f32")
        if bad_s.any():
            at = tuple(np.argwhere(bad_s)[0])
            failures.append(f"{case.name}: {int(bad_s.sum())} scales differ, first at {at}: {to_numpy(scales)[at]!r} vs {s_ref[at]!r}")
        if not ((got[:, :, :, [0, T + 1]].view(np.uint8) == GUARD_Q).all() and (to_numpy(sc)[:, [0, T + 1]] == GUARD_S).all()):
            failures.append(f"{case.name}: guard token or guard scale overwritten")
    assert not failures, failures


@pytest.mark.parametrize("row", QROWS, ids=[r[0] for r in QROWS])
def test_quant_edges(row):
    _check_row(row, lambda dims, dt, kind, given: C.quant_cases(dims, dt, kind, given_table=given, max_chunks=1))


@pytest.mark.parametrize("row", QROWS, ids=[r[0] for r in QROWS])
def test_quant_nonfinite(row):
    """A poison must not reroute a call (the kernel log is the row's), must not reach a guard token or guard scale, and
    must leave the clean tokens that share its tile, wave or workgroup with the oracle's bits."""
    _check_row(row, lambda dims, dt, kind, given: C.nonfinite_cases(dims, dt, kind, given_table=given))


AROWS = [r for r in ROWS if r[1] in ("absmax", "absmax_acc")]


@pytest.mark.parametrize("row", AROWS, ids=[r[0] for r in AROWS])
def test_absmax_nonfinite(row):
    """kvq_absmax_tokens[_acc] on the family: NaN for a slice with a NaN, else +inf for one with an inf, the oracle's bits
    for the clean ones; the accumulating call onto a table that already holds NaN, +inf, a finite value above the data
    and one below keeps the table's NaN. The table sits between two guard rows."""
    from efficient_llm_inference_amd import _lib
    from tests.test_gpu_quant_routing import _call
    name, entry, dtype, dims, layout, knobs, with_ws, want, _rc, _check = row
    G, B, H, T, D = dims
    old = np.resize(np.array([np.nan, np.inf, 1e9, 2.0 ** -20], np.float32), (G, T))
    failures = []
    for case in C.nonfinite_cases(dims, DT[dtype], "int8", given_table=False):
        x = _place(layout, to_torch(case.x, DT[dtype], device="cpu").view(TORCH[dtype]))
        buf = torch.full((G + 2, T), GUARD_S, dtype=torch.float32, device="cuda")
        table = buf[1:G + 1]
        if entry == "absmax_acc":
            table.copy_(torch.from_numpy(old))
        with tunables(**knobs):
            _lib.kernel_log_clear()
            rc = _call(entry, x, None, table, None, None)
            torch.cuda.synchronize()
            log = _lib.kernel_log()
        assert rc == 0 and log == want, (case.name, rc, log)
        am = C.data_absmax(case.x, case.dtype)
        ref = np.maximum(old, am) if entry == "absmax_acc" else am
        got = to_numpy(buf)
        bad = C.float_mismatch(got[1:G + 1], ref, "f32")
        if bad.any() or (C.absmax_class(got[1:G + 1]) != C.absmax_class(ref)).any():
            at = tuple(np.argwhere(bad)[0]) if bad.any() else ()
            failures.append(f"{case.name}: {int(bad.sum())} entries differ, first at {at}: {got[1:G + 1][at]!r} vs {ref[at]!r}")
        if not (got[[0, G + 1]] == GUARD_S).all():
            failures.append(f"{case.name}: guard row overwritten")
    assert not failures, failures


# ------------------------------------------------------------------------------------------------------ dequantise

def _dequant_ref(q, s, kind, D, out):
    with np.errstate(over="ignore"):
        return O.dequantize_tokens(q, s, kind, D, out)


@pytest.mark.parametrize("route", ["fast", "generic"])
@pytest.mark.parametrize("out_dtype", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("kind", ["int8", "int4"])
def test_dequant_tokens_edges(kind, out_dtype, route):
    from efficient_llm_inference_amd import _lib, kernels
    for cname, q_np, s_np in C.dequant_code_cases(kind, out_dtype):
        G, B, H, T, Dq = q_np.shape
        D = Dq if kind == "int8" else 2 * Dq
        q = torch.from_numpy(q_np).cuda()
        s = torch.from_numpy(s_np).cuda()
        pad = 0 if route == "fast" else 8  # a token stride of D + 8 in the output takes the generic kernel
        big = torch.zeros(G, B, H, T, D + pad, dtype={"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}[out_dtype],
                          device="cuda")
        out = big[..., :D]
        _lib.kernel_log_clear()
        kernels.dequant_tokens(q, s, out, kind)
        torch.cuda.synchronize()
        log = _lib.kernel_log()
        assert len(log) == 1 and log[0].startswith(f"dequant_tokens_{route}_k<"), (cname, log)
        ref = _dequant_ref(q_np, s_np, kind, D, out_dtype)
        if np.isfinite(s_np).all():
            assert np.array_equal(bits(out), np.ascontiguousarray(ref).view(np.uint8)), cname
        else:  # NaN, +inf, -inf scales: any NaN for the oracle's NaN (code 0 times inf, anything times NaN), its bits for ±inf
            assert C.same_floats(to_numpy(out), ref, out_dtype), cname
            assert C.is_nan_bits(C.raw_bits(ref, out_dtype), out_dtype).any() and not C.is_nan_bits(C.raw_bits(ref, out_dtype), out_dtype).all()
        if pad:
            assert (to_numpy(big[..., D:]).view(np.uint8) == 0).all()


# (route, kind, elements): the flat entry points pick their kernel by size and alignment
FLAT = [("chunk", "int8", 1 << 20), ("vec", "int8", 4096), ("scalar", "int8", 4095),
        ("chunk", "int4", 1 << 20), ("vec", "int4", 4096), ("scalar", "int4", 4094)]
FLAT_KERNEL = {"chunk": "dequant_flat_chunk_k<", "vec": "dequant_flat_vec_k<", "scalar": "dequant_i"}


@pytest.mark.parametrize("route,kind,n", FLAT, ids=[f"{k}_{r}" for r, k, _ in FLAT])
def test_dequant_flat_edges(route, kind, n):
    from efficient_llm_inference_amd import _lib, kernels
    (_, q_np, s_np), (_, _, s_bad) = C.dequant_code_cases(kind, "f16")
    codes = q_np.reshape(-1).view(np.uint8)
    if kind == "int8":
        flat = np.resize(codes, n).view(np.int8)
    else:
        last = 64 if route != "scalar" else 63          # scalar: an odd last dim leaves a pad column to zero
        packed_last = (last + 1) // 2
        flat = np.resize(codes, n // 2 // packed_last * packed_last).reshape(-1, packed_last)
    qt = torch.from_numpy(flat).cuda()
    failures = []
    for s in list(s_np.reshape(-1)) + list(s_bad.reshape(-1)[:3]):  # ... and NaN, +inf, -inf
        _lib.kernel_log_clear()
        out = kernels.dequant_i8_flat(qt, float(s)) if kind == "int8" else kernels.dequant_i4_flat(qt, float(s), last)
        torch.cuda.synchronize()
        log = _lib.kernel_log()
        assert len(log) == 1 and log[0].startswith(FLAT_KERNEL[route]), log
        with np.errstate(over="ignore", invalid="ignore"):
            ref = O.dequantize_int8_per_tensor(flat, np.float32(s), "f16") if kind == "int8" else \
                O.dequant_int4_packed_kernel_full(flat, np.float32(s), last)
        same = np.array_equal(bits(out), np.ascontiguousarray(ref).view(np.uint8)) if np.isfinite(s) else \
            C.same_floats(to_numpy(out), ref, "f16")
        if not same:
            failures.append(float(s))
    assert not failures, f"scales {failures}"


# ------------------------------------------------------------------------------- appends with their own quantise code
# The decode step quantises its new token inside the attention merge launch (csrc/attn/merge.inc), with routines of its
# own: quant_new_token_regs (slices of at most 8,192 elements, fast merge), quant_new_token_parts (larger slices: one
# workgroup per 8,192 elements) and quant_new_token_block (the chained merge, or parts switched off). The slice size and
# the tunables pick the routine; the kernel log names the merge kernel that ran it. Every family of quant_cases (eps
# included) goes through each, one token per step, into slot T of a store with guard slots on both sides.
NT, T0 = 4, 2  # tokens per case (one decode step each), stored tokens before them
DECODE = [  # (id, entry, B, Hkv, D, tunables, merge kernel prefix, routine)
    ("step_fast_regs", "step", 1, 8, 128, {}, "decode_attn_merge_fast_k<", "regs"),
    ("step_fast_parts", "step", 16, 8, 128, {}, "decode_attn_merge_fast_k<", "parts"),
    ("step_fast_block", "step", 16, 8, 128, {"attn_new_token_parts": 0}, "decode_attn_merge_fast_k<", "block"),
    ("step_chained_block", "step", 1, 8, 128, {"attn_merge_fast": 0}, "decode_attn_merge_k", "block"),
    ("step_chained_parts", "step", 16, 8, 128, {"attn_merge_fast": 0}, "decode_attn_merge_k", "parts"),
    ("dev_regs", "dev", 1, 8, 128, {}, "decode_attn_merge_fast_k<", "regs"),
    ("dev_parts", "dev", 16, 8, 128, {}, "decode_attn_merge_fast_k<", "parts"),
]


def _slot_ref(case, kind, t):
    q, s = C.reference(C.Case(case.name, case.x[:, :, :, t:t + 1], case.dtype, case.eps), kind)
    return q[0, :, :, 0], s[0, 0]


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("kind", ["int8", "int4"])
@pytest.mark.parametrize("row", DECODE, ids=[r[0] for r in DECODE])
def test_decode_step_append_edges(row, kind, dtype):
    from efficient_llm_inference_amd import _lib, kernels
    name, entry, B, Hkv, D, knobs, merge, routine = row
    n = B * Hkv * D
    assert (n <= 8192) == (routine == "regs" or name == "step_chained_block")  # the slice size picks the routine
    Hq, cap = Hkv, T0 + NT + 1
    Dq = kernels.packed_dim(kind, D)
    tdt = TORCH[F16 if dtype == "f16" else BF16]
    q = torch.zeros(B, Hq, D, dtype=tdt, device="cuda")
    out = torch.empty_like(q)
    ws = torch.empty(kernels.decode_attn_workspace_cap(B, Hq, Hkv, cap, D), dtype=torch.float32, device="cuda")
    t_dev = torch.zeros(1, dtype=torch.int32, device="cuda")
    stores = [torch.empty(B, Hkv, cap, Dq, dtype=kernels.QDTYPE[kind], device="cuda") for _ in range(2)]
    scs = [torch.empty(cap, dtype=torch.float32, device="cuda") for _ in range(2)]
    failures = []
    for case in C.quant_cases((1, B, Hkv, NT, D), dtype, kind, given_table=False, max_chunks=1):
        for st, sc in zip(stores, scs):
            st.view(torch.uint8).fill_(GUARD_Q)
            st[:, :, :T0].view(torch.uint8).fill_(0x88 if kind == "int4" else 0)  # stored tokens: code 0, scale 1
            sc.fill_(GUARD_S)
            sc[:T0] = 1.0
        x = to_torch(case.x, dtype, device="cuda")[0]  # [B, Hkv, NT, D]
        plan = kernels.DecodeStepPlan(q, stores[0], scs[0], kind, stores[1], scs[1], kind, case.eps)
        with tunables(**knobs):
            for t in range(NT):
                kn = x[:, :, t].contiguous()
                _lib.kernel_log_clear()
                if entry == "step":
                    kernels.decode_step(plan, q, kn, kn, T0 + t, out, ws, D ** -0.5)
                else:
                    t_dev.fill_(T0 + t)
                    kernels.decode_step_dev(plan, q, kn, kn, t_dev, cap - 1, out, ws, D ** -0.5)
                torch.cuda.synchronize()
                log = _lib.kernel_log()
                assert any(k.startswith(merge) for k in log), (case.name, log)
        for w, (st, sc) in enumerate(zip(stores, scs)):
            got, gs = to_numpy(st), to_numpy(sc)
            for t in range(NT):
                q_ref, s_ref = _slot_ref(case, kind, t)
                if not np.array_equal(got[:, :, T0 + t], q_ref):
                    failures.append(f"{case.name} {'KV'[w]} token {t}: {int((got[:, :, T0 + t] != q_ref).sum())} bytes differ")
                if gs[T0 + t].view(np.uint32) != np.float32(s_ref).view(np.uint32):
                    failures.append(f"{case.name} {'KV'[w]} token {t}: scale {gs[T0 + t]} vs {s_ref}")
            if not ((got[:, :, T0 + NT:].view(np.uint8) == GUARD_Q).all() and (gs[T0 + NT:] == GUARD_S).all()):
                failures.append(f"{case.name} {'KV'[w]}: guard slot overwritten")
    assert not failures, failures[:10]


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("kind", ["int8", "int4"])
@pytest.mark.parametrize("row", DECODE, ids=[r[0] for r in DECODE])
def test_decode_step_append_nonfinite(row, kind, dtype):
    """The non-finite family through the regs, parts and block routines: every token of a case is one decode step at
    T0 stored tokens (code 0, scale 1) into slot T0 of both stores, re-initialised per step so that a poisoned token never
    becomes a key of a later step. Slot T0 against the oracle (codes exact, scale by the comparison rule), the guard slots
    behind it untouched, and on a step whose new token is clean the attention output finite."""
    from efficient_llm_inference_amd import _lib, kernels
    name, entry, B, Hkv, D, knobs, merge, routine = row
    Hq, cap = Hkv, T0 + 3
    Dq = kernels.packed_dim(kind, D)
    tdt = TORCH[F16 if dtype == "f16" else BF16]
    q = torch.zeros(B, Hq, D, dtype=tdt, device="cuda")
    out = torch.empty_like(q)
    ws = torch.empty(kernels.decode_attn_workspace_cap(B, Hq, Hkv, cap, D), dtype=torch.float32, device="cuda")
    t_dev = torch.full((1,), T0, dtype=torch.int32, device="cuda")
    stores = [torch.empty(B, Hkv, cap, Dq, dtype=kernels.QDTYPE[kind], device="cuda") for _ in range(2)]
    scs = [torch.empty(cap, dtype=torch.float32, device="cuda") for _ in range(2)]
    failures = []
    for case in C.nonfinite_cases((1, B, Hkv, NT, D), dtype, kind, given_table=False):
        x = to_torch(case.x, dtype, device="cuda")[0]  # [B, Hkv, NT, D]
        clean = np.isfinite(C.widen(case.x, dtype)).all(axis=(0, 1, 2, 4))  # [NT]
        assert not clean.all()
        plan = kernels.DecodeStepPlan(q, stores[0], scs[0], kind, stores[1], scs[1], kind, case.eps)
        for t in range(NT):
            for st, sc in zip(stores, scs):
                st.view(torch.uint8).fill_(GUARD_Q)
                st[:, :, :T0].view(torch.uint8).fill_(0x88 if kind == "int4" else 0)
                sc.fill_(GUARD_S)
                sc[:T0] = 1.0
            kn = x[:, :, t].contiguous()
            with tunables(**knobs):
                _lib.kernel_log_clear()
                if entry == "step":
                    kernels.decode_step(plan, q, kn, kn, T0, out, ws, D ** -0.5)
                else:
                    kernels.decode_step_dev(plan, q, kn, kn, t_dev, cap - 1, out, ws, D ** -0.5)
                torch.cuda.synchronize()
                log = _lib.kernel_log()
            assert any(k.startswith(merge) for k in log), (case.name, log)
            q_ref, s_ref = _slot_ref(case, kind, t)
            for w, (st, sc) in enumerate(zip(stores, scs)):
                got, gs = to_numpy(st), to_numpy(sc)
                if not np.array_equal(got[:, :, T0], q_ref):
                    bad = np.argwhere(got[:, :, T0] != q_ref)
                    failures.append(f"{case.name} {'KV'[w]} token {t}: {len(bad)} bytes differ, first at {tuple(bad[0])}: "
                                    f"{got[:, :, T0][tuple(bad[0])]} vs {q_ref[tuple(bad[0])]}")
                if not C.same_floats(gs[T0:T0 + 1], np.float32(s_ref).reshape(1)):
                    failures.append(f"{case.name} {'KV'[w]} token {t}: scale {gs[T0]!r} vs {s_ref!r}")
                if not ((got[:, :, T0 + 1:].view(np.uint8) == GUARD_Q).all() and (gs[T0 + 1:] == GUARD_S).all()):
                    failures.append(f"{case.name} {'KV'[w]} token {t}: guard slot overwritten")
            if clean[t] and not np.isfinite(to_numpy(out.float())).all():
                failures.append(f"{case.name} token {t}: attention output not finite on a clean step")
    assert not failures, failures[:10]


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("kind", ["int8", "int4"])
def test_extend_append_edges(kind, dtype):
    """QuantizedKVCache.extend(append=True): the chunk is quantised into the layer's K and V groups by kvq_quant_*_tokens
    through the store window (the one-wave tile at 8 x 128). The cache has no public eps; the eps cases set the stores'."""
    _check_extend(kind, dtype, C.quant_cases((1, 1, 8, 12, 128), dtype, kind, given_table=False, max_chunks=1))


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("kind", ["int8", "int4"])
def test_extend_append_nonfinite(kind, dtype):
    """the same append on the non-finite family (scales by the comparison rule)"""
    _check_extend(kind, dtype, C.nonfinite_cases((1, 1, 8, 12, 128), dtype, kind, given_table=False))


def _check_extend(kind, dtype, cases):
    import efficient_llm_inference_amd as E
    from efficient_llm_inference_amd import _lib
    B, Hkv, S, D = 1, 8, 12, 128
    idt = F16 if dtype == "f16" else BF16
    want = tile(idt, 8 if kind == "int8" else 4, 8, 16, 4, 0)
    failures = []
    for case in cases:
        x = to_torch(case.x, dtype, device="cuda")[0]
        qc = E.QuantizedKVCache(1, kind, compute_dtype=TORCH[idt])
        qc._k.eps = qc._v.eps = case.eps
        _lib.kernel_log_clear()
        qc.extend(0, torch.zeros(B, 2 * Hkv, S, D, dtype=TORCH[idt], device="cuda"), x, x)
        torch.cuda.synchronize()
        log = _lib.kernel_log()
        assert want in log, (case.name, log)
        q_ref, s_ref = C.reference(case, kind)
        for w, st in enumerate((qc._k, qc._v)):
            if not (np.array_equal(to_numpy(st.q[:1, :, :, :S]), q_ref) and C.same_floats(to_numpy(st.scales[:1, :S]), s_ref)):
                failures.append(f"{case.name} {'KV'[w]}")
    assert not failures, failures


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("kind", ["int8", "int4"])
def test_sharded_joint_append_edges(kind, dtype):
    """sharding.quantize_kv_batch_sharded on one rank, two_phase: ONE abs-max launch over the 2G tensors of K and V (the
    few-token kernel), then the phase-2 tile walk per set; both sets compared with the oracle on the whole slice."""
    _check_sharded_joint(kind, dtype, C.quant_cases((8, 8, 8, 1, 128), dtype, kind, given_table=False, max_chunks=1))


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("kind", ["int8", "int4"])
def test_sharded_joint_append_nonfinite(kind, dtype):
    """the same one-rank joint append on the non-finite family (what a collective's MAX does with a NaN across ranks is
    the collective library's: DESIGN.md §4)"""
    _check_sharded_joint(kind, dtype, C.nonfinite_cases((8, 8, 8, 1, 128), dtype, kind, given_table=False))


def _check_sharded_joint(kind, dtype, cases):
    from efficient_llm_inference_amd import _lib, sharding
    G, B, Hkv, T, D = 8, 8, 8, 1, 128
    idt = F16 if dtype == "f16" else BF16
    bits_ = 8 if kind == "int8" else 4
    want = [f"absmax_fewtokens_k<{idt}, 16>", f"quant_tile_k<{idt}, {bits_}, 8, 16, 4, 2>"]
    failures = []
    for case in cases:
        xk = to_torch(case.x, dtype, device="cuda")
        xv = xk.clone()
        assert sharding.kv_joint_table_ok(G, T)
        _lib.kernel_log_clear()
        (qk, sk), (qv, sv) = sharding.quantize_kv_batch_sharded(xk, xv, (kind, kind), case.eps, two_phase=True)
        torch.cuda.synchronize()
        log = _lib.kernel_log()
        assert log == want, (case.name, log)
        q_ref, s_ref = C.reference(case, kind)
        for w, (qq, ss) in enumerate(((qk, sk), (qv, sv))):
            if not (np.array_equal(to_numpy(qq), q_ref) and C.same_floats(to_numpy(ss), s_ref)):
                failures.append(f"{case.name} {'KV'[w]}")
    assert not failures, failures
