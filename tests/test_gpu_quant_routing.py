"""Which kernels each quantise entry point launches, shape by shape: one row per routing family and sub-case (see the
routing table above quant_route / split_route in csrc/kvq_quant.hip). Each row asserts the exact kvq_kernel_log list of
one call: distinct kernels, in first-launch order. Bytes are checked against the oracle only where the parity tests do
not already cover the row."""
import numpy as np
import pytest
import torch

from oracle import kvq_oracle as O
from tests.util import bits, to_numpy, tunables

pytestmark = pytest.mark.gpu

F16, BF16, F32 = 0, 1, 2
TORCH = {F16: torch.float16, BF16: torch.bfloat16, F32: torch.float32}


def tile(idt, b, r, dv, tt, phase):
    return f"quant_tile_k<{idt}, {b}, {r}, {dv}, {tt}, {phase}>"


def fused(idt, b, rowu, lds, full, blk, regmax=0):
    f = lambda v: "true" if v else "false"
    return f"quant_tokens_fused_k<{idt}, {b}, {f(rowu)}, {f(lds)}, {f(full)}, {blk}, {regmax}, 8, false, true, true>"


def wide(idt, b):
    return f"quant_wide_k<{idt}, {b}, 1024, 16>"


def sweep(idt, b):
    return f"quant_tokens_sweep_k<{idt}, {b}, false>"


def generic(idt, b):
    return [f"absmax_tokens_generic_k<{idt}>", f"quant_tokens_generic_k<{idt}, {b}>"]


# (id, entry, dtype, (G, B, H, T, D), layout, tunables, workspace, expected kernel log, expected rc, check bytes)
# entry: i8 / i4 = kvq_quant_i8/i4_tokens, absmax / absmax_acc = kvq_absmax_tokens[_acc], from8 / from4 =
# kvq_quant_tokens_from_absmax. layout: contig [G,B,H,T,D]; bstride = every other batch row of a [G,2B,H,T,D] tensor;
# misaligned = G separate [B,H,T,D] tensors, the last one (in the second launch chunk) 2 bytes off a 16-byte boundary.
ROWS = [
    ("tile128", "i4", F16, (2, 1, 8, 33, 128), "contig", {}, True, [tile(F16, 4, 8, 16, 4, 0)], 0, False),
    ("tile64", "i8", BF16, (2, 2, 4, 16, 64), "contig", {}, True, [tile(BF16, 8, 8, 8, 8, 0)], 0, False),
    ("tile64_r12", "i4", F16, (1, 1, 12, 5, 64), "contig", {}, True, [tile(F16, 4, 12, 8, 8, 0)], 0, False),
    ("wide", "i8", F16, (1, 32, 8, 4, 128), "contig", {}, True, [wide(F16, 8)], 0, False),
    ("wide_bstride", "i4", BF16, (1, 32, 8, 4, 128), "bstride", {}, True, [wide(BF16, 4)], 0, False),
    ("split_few", "i8", F16, (1, 256, 8, 2, 128), "contig", {}, True,
     ["absmax_fewtokens_k<0, 16>", tile(F16, 8, 8, 16, 4, 2)], 0, True),
    ("split_walk", "i4", BF16, (1, 32, 8, 32, 128), "contig", {"quant_wide": 0}, True,
     [tile(BF16, 8, 8, 16, 4, 1), tile(BF16, 4, 8, 16, 4, 2)], 0, False),
    ("sweep_anydv", "i8", F16, (2, 1, 8, 5, 24), "contig", {}, True, [sweep(F16, 8)], 0, False),
    ("sweep_no_ws", "i8", F16, (1, 256, 8, 2, 128), "contig", {}, False, [sweep(F16, 8)], 0, True),
    ("wave_regmax", "i8", F16, (1, 1, 8, 22, 128), "contig", {"quant_tile": 0}, True,
     [fused(F16, 8, 1, 1, 1, 64, 1), fused(F16, 8, 1, 1, 0, 64)], 0, False),
    ("wave_full", "i4", BF16, (1, 1, 4, 43, 128), "contig", {}, True,
     [fused(BF16, 4, 1, 1, 1, 64), fused(BF16, 4, 1, 1, 0, 64)], 0, False),
    ("wave_ragged", "i8", F16, (1, 1, 6, 9, 128), "contig", {}, True, [fused(F16, 8, 1, 1, 0, 64)], 0, False),
    ("blk256_lds", "i8", F32, (1, 1, 4, 43, 128), "contig", {}, True,
     [fused(F32, 8, 1, 1, 1, 256), fused(F32, 8, 0, 1, 0, 256)], 0, False),
    ("blk256_direct", "i4", F16, (1, 1, 4, 43, 128), "contig", {"quant_block": 256, "quant_direct_stores": 1}, True,
     [fused(F16, 4, 0, 0, 0, 256)], 0, False),
    ("generic_odd_d", "i8", F16, (2, 1, 8, 3, 7), "contig", {}, True, generic(F16, 8), 0, False),
    ("generic_forced", "i4", BF16, (1, 1, 8, 4, 128), "contig", {"quant_force_two_pass": 1}, True, generic(BF16, 4), 0, False),
    ("generic_f32_big", "i8", F32, (1, 32, 8, 2, 128), "contig", {}, True, generic(F32, 8), 0, False),
    ("chunk_fallback", "i8", F16, (130, 1, 8, 4, 128), "misaligned", {}, True,
     [fused(F16, 8, 1, 1, 1, 64, 1)] + generic(F16, 8), 0, True),
    ("chunk_fallback_no_ws", "i8", F16, (130, 1, 8, 4, 128), "misaligned", {}, False, [fused(F16, 8, 1, 1, 1, 64, 1)], -1, False),
    ("absmax_walk", "absmax", F16, (2, 4, 8, 32, 128), "contig", {}, True, [tile(F16, 8, 8, 16, 4, 1)], 0, True),
    ("absmax_walk_8rows", "absmax", F16, (1, 1, 8, 1, 128), "contig", {}, True, [tile(F16, 8, 8, 16, 4, 1)], 0, True),
    ("absmax_few", "absmax", BF16, (2, 4, 8, 1, 128), "contig", {}, True, ["absmax_fewtokens_k<1, 16>"], 0, True),
    ("absmax_acc_few", "absmax_acc", F16, (2, 4, 8, 3, 128), "contig", {}, True, ["absmax_fewtokens_k<0, 16>"], 0, True),
    ("absmax_acc_walk", "absmax_acc", F16, (1, 4, 8, 32, 128), "contig", {}, True, [tile(F16, 8, 8, 16, 4, 1)], 0, True),
    ("absmax_vec", "absmax", F32, (2, 2, 4, 5, 128), "contig", {}, True, ["absmax_tokens_tile_k<2>"], 0, True),
    ("absmax_generic", "absmax", F16, (2, 1, 4, 3, 7), "contig", {}, True, ["absmax_tokens_generic_k<0>"], 0, True),
    ("absmax_chunk_fallback", "absmax", F16, (130, 1, 2, 4, 64), "misaligned", {}, True,
     ["absmax_tokens_tile_k<0>", "absmax_tokens_generic_k<0>"], 0, True),
    ("from_tile", "from4", F16, (2, 4, 8, 3, 128), "contig", {}, True, [tile(F16, 4, 8, 16, 4, 2)], 0, False),
    ("from_vec", "from8", BF16, (2, 2, 4, 5, 64), "contig", {}, True, ["quant_tokens_scaled_tile_k<1, 8>"], 0, False),
    ("from_generic", "from4", F16, (1, 1, 4, 3, 7), "contig", {}, True, ["quant_tokens_generic_k<0, 4>"], 0, False),
]


def _input(layout, dtype, dims, seed):
    G, B, H, T, D = dims
    gen = torch.Generator().manual_seed(seed)
    full = torch.randn((G, 2 * B if layout == "bstride" else B, H, T, D), generator=gen).to(TORCH[dtype])
    if layout == "contig":
        return full.cuda(), full
    if layout == "bstride":
        return full.cuda()[:, ::2], full[:, ::2]
    xs = [full[g].cuda() for g in range(G - 1)]
    n = B * H * T * D
    buf = torch.empty(n + 8, dtype=TORCH[dtype], device="cuda")
    last = buf[1:1 + n].view(B, H, T, D)  # 2 or 4 bytes past a 16-byte boundary
    last.copy_(full[G - 1])
    assert last.data_ptr() % 16 != 0
    return xs + [last], full


def _call(entry, x, ws, table, q, scales):
    from efficient_llm_inference_amd import _lib, kernels
    from efficient_llm_inference_amd._lib import byref, c_void_p
    base, arr, ist, (G, B, H, T, D), dt, dev, _keep = kernels._in_views(x)
    lib, dims, dcode = _lib.load(), _lib.dims5(G, B, H, T, D), _lib.dtype_code(dt)
    wsp = c_void_p(ws.data_ptr()) if ws is not None else None
    if entry in ("i8", "i4"):
        fn = lib.kvq_quant_i8_tokens if entry == "i8" else lib.kvq_quant_i4_tokens
        return kernels._launch(dev, fn, base, arr, byref(ist), dcode, c_void_p(q.data_ptr()), byref(_lib.strides4(q)),
                               c_void_p(scales.data_ptr()), scales.stride(0), wsp, 1e-8, byref(dims))
    if entry in ("absmax", "absmax_acc"):
        fn = lib.kvq_absmax_tokens_acc if entry == "absmax_acc" else lib.kvq_absmax_tokens
        return kernels._launch(dev, fn, base, arr, byref(ist), dcode, c_void_p(table.data_ptr()), byref(dims))
    return kernels._launch(dev, lib.kvq_quant_tokens_from_absmax, 8 if entry == "from8" else 4, base, arr, byref(ist), dcode,
                           c_void_p(q.data_ptr()), byref(_lib.strides4(q)), c_void_p(scales.data_ptr()), scales.stride(0),
                           c_void_p(table.data_ptr()), 1e-8, byref(dims))


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_quant_routing(row):
    from efficient_llm_inference_amd import _lib, kernels
    name, entry, dtype, dims, layout, knobs, with_ws, want, want_rc, check = row
    G, B, H, T, D = dims
    x, x_cpu = _input(layout, dtype, dims, seed=len(name) * 7919 + G + T)
    kind = "int4" if entry in ("i4", "from4") else "int8"
    Dq = kernels.packed_dim(kind, D)
    q = torch.zeros(G, B, H, T, Dq, dtype=kernels.QDTYPE[kind], device="cuda")
    scales = torch.zeros(G, T, dtype=torch.float32, device="cuda")
    ws = torch.full((G * T,), -1.0, dtype=torch.float32, device="cuda") if with_ws else None
    amax = x_cpu.float().abs().amax(dim=(1, 2, 4))  # [G, T]
    old = torch.rand(G, T, generator=torch.Generator().manual_seed(3)) * 4.0  # what an accumulating call keeps
    table = (old if entry == "absmax_acc" else amax if entry.startswith("from") else torch.full((G, T), -1.0)).cuda()
    torch.cuda.synchronize()
    with tunables(**knobs):
        _lib.kernel_log_clear()
        rc = _call(entry, x, ws, table, q, scales)
        torch.cuda.synchronize()
        log = _lib.kernel_log()
    assert rc == want_rc, (rc, _lib.load().kvq_last_error_string())
    assert log == want, log
    if not check:
        return
    if entry.startswith("absmax"):
        ref = torch.maximum(amax, old) if entry == "absmax_acc" else amax
        assert torch.equal(table.cpu(), ref)
        return
    q_ref, _, s32_ref = O.quantize_tokens(x_cpu.contiguous().numpy(), kind)  # (fp16 rows only)
    assert np.array_equal(to_numpy(q), q_ref) and np.array_equal(bits(scales), bits(s32_ref))
