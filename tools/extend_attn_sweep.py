#!/usr/bin/env python3
"""kvq_extend_attn (multi-token causal attention over the quantised store) on the two shapes it is built for, one JSON
line per row:

  verify   speculative-decoding verify: Llama-3-8B grouping (B 8, Hq 32, Hkv 8, D 128), 16,384 stored tokens, INT8 K +
           INT4 V, S = 1 / 4 / 16 query tokens; kvq_decode_attn at the same shape in the same run as the yardstick
  prefill  a chunk of S = 512 tokens behind 16,384 stored ones at batch 1 (same heads, same store); effective TFLOP/s =
           4 * B * Hq * S * (T + (S + 1) / 2) * D / time. Also the alternative the feature replaces: dequant_tokens of the
           store to fp16, cat the chunk, torch SDPA with the lower-right causal mask (for information)

Per call: the attention kernel's own duration (kvq_time_next_launch events on its dispatch) and the wall time of the
whole call (attention + merge launch) averaged over back-to-back calls on one stream."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402


def _time(fn, n=50, warm=5):
    """(first-launch kernel us via events, wall us per call) over n calls"""
    from efficient_llm_inference_amd import _lib
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    e1.record()
    ks = []
    for _ in range(10):
        with _lib.timed_launch(e0, e1):
            fn()
        e1.synchronize()
        ks.append(e0.elapsed_time(e1) * 1e3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return round(sorted(ks)[len(ks) // 2], 2), round((time.perf_counter() - t0) / n * 1e6, 2)


def main():
    from efficient_llm_inference_amd import _lib
    from efficient_llm_inference_amd import kernels as K
    dev = torch.device("cuda:0")
    Hq, Hkv, D, T = 32, 8, 128, 16384
    sm = D ** -0.5
    torch.manual_seed(0)

    def store(B):
        cap = T + 16
        ks = torch.randint(-127, 128, (B, Hkv, cap, D), device=dev, dtype=torch.int8)
        vs = torch.randint(0, 256, (B, Hkv, cap, D // 2), device=dev, dtype=torch.uint8)
        ksc = torch.rand(cap, device=dev) * 0.01 + 0.001
        vsc = torch.rand(cap, device=dev) * 0.01 + 0.001
        return ks, vs, ksc, vsc

    def kernels_of(fn):
        _lib.kernel_log_clear()
        fn()
        torch.cuda.synchronize()
        return [k.split("(")[0] for k in _lib.kernel_log()]

    # speculative verify
    B = 8
    ks, vs, ksc, vsc = store(B)
    q1 = torch.randn(B, Hq, D, device=dev, dtype=torch.float16)
    kn1 = torch.randn(B, Hkv, D, device=dev, dtype=torch.float16)
    vn1 = torch.randn(B, Hkv, D, device=dev, dtype=torch.float16)
    o1 = torch.empty_like(q1)
    wsd = torch.empty(K.decode_attn_workspace(B, Hq, Hkv, T, D), device=dev)
    dec = lambda: K.decode_attn(q1, ks, ksc, "int8", vs, vsc, "int4", T, o1, wsd, sm, kn1, vn1)  # noqa: E731
    dk, dw = _time(dec)
    store_mb = B * Hkv * T * (D + D // 2) / 1e6
    print(json.dumps({"workload": "verify", "op": "decode_attn", "B": B, "Hq": Hq, "Hkv": Hkv, "D": D, "T": T,
                      "kernel_us": dk, "call_us": dw, "store_MB": round(store_mb, 1), "kernels": kernels_of(dec)}), flush=True)
    for S in (1, 4, 16):
        q = torch.randn(B, S, Hq, D, device=dev, dtype=torch.float16).transpose(1, 2)
        kn = torch.randn(B, S, Hkv, D, device=dev, dtype=torch.float16).transpose(1, 2)
        vn = torch.randn(B, S, Hkv, D, device=dev, dtype=torch.float16).transpose(1, 2)
        out = torch.empty(B, S, Hq, D, device=dev, dtype=torch.float16).transpose(1, 2)
        ws = torch.empty(max(1, K.extend_attn_workspace(B, Hq, Hkv, T, S, D)), device=dev)
        fn = lambda: K.extend_attn(q, ks, ksc, "int8", vs, vsc, "int4", T, kn, vn, out, ws, sm)  # noqa: E731
        ek, ew = _time(fn)
        print(json.dumps({"workload": "verify", "op": "extend_attn", "B": B, "Hq": Hq, "Hkv": Hkv, "D": D, "T": T, "S": S,
                          "kernel_us": ek, "call_us": ew, "x_decode_call": round(ew / dw, 2),
                          "store_TBps": round(store_mb / ew, 2), "kernels": kernels_of(fn)}), flush=True)
    del ks, vs, ksc, vsc

    # chunked prefill
    B, S = 1, 512
    ks, vs, ksc, vsc = store(B)
    q = torch.randn(B, S, Hq, D, device=dev, dtype=torch.float16).transpose(1, 2)
    kn = torch.randn(B, S, Hkv, D, device=dev, dtype=torch.float16).transpose(1, 2)
    vn = torch.randn(B, S, Hkv, D, device=dev, dtype=torch.float16).transpose(1, 2)
    out = torch.empty(B, S, Hq, D, device=dev, dtype=torch.float16).transpose(1, 2)
    ws = torch.empty(max(1, K.extend_attn_workspace(B, Hq, Hkv, T, S, D)), device=dev)
    fn = lambda: K.extend_attn(q, ks, ksc, "int8", vs, vsc, "int4", T, kn, vn, out, ws, sm)  # noqa: E731
    ek, ew = _time(fn, n=20)
    flop = 4.0 * B * Hq * S * (T + (S + 1) / 2) * D
    print(json.dumps({"workload": "prefill", "op": "extend_attn", "B": B, "Hq": Hq, "Hkv": Hkv, "D": D, "T": T, "S": S,
                      "kernel_us": ek, "call_us": ew, "GFLOP": round(flop / 1e9, 1),
                      "TFLOPs_call": round(flop / ew / 1e6, 1), "kernels": kernels_of(fn)}), flush=True)

    # the alternative: dequantise the store to fp16, cat the chunk, SDPA with the lower-right causal mask
    kd = torch.empty(1, B, Hkv, T, D, device=dev, dtype=torch.float16)
    vd = torch.empty_like(kd)
    mask = torch.ones(S, T + S, device=dev, dtype=torch.bool)
    mask[:, T:] = torch.ones(S, S, device=dev, dtype=torch.bool).tril()

    def alt():
        K.dequant_tokens(ks[None, :, :, :T], ksc[None, :T], kd, "int8")
        K.dequant_tokens(vs[None, :, :, :T], vsc[None, :T], vd, "int4")
        kf = torch.cat([kd[0], kn], dim=2)
        vf = torch.cat([vd[0], vn], dim=2)
        return torch.nn.functional.scaled_dot_product_attention(q, kf, vf, attn_mask=mask, scale=sm, enable_gqa=True)

    for _ in range(3):
        alt()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        alt()
    torch.cuda.synchronize()
    aw = (time.perf_counter() - t0) / 10 * 1e6
    print(json.dumps({"workload": "prefill", "op": "dequant_tokens+cat+sdpa", "B": B, "T": T, "S": S,
                      "call_us": round(aw, 1), "TFLOPs_call": round(flop / aw / 1e6, 1)}), flush=True)


if __name__ == "__main__":
    main()
