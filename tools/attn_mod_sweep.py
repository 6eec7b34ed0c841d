#!/usr/bin/env python3
"""Logit soft-capping and attention sinks in decode attention over the quantised store (kvq_decode_step_ex):
per-layer-call time with a cap only, sinks only and both against the same call with both off, which is the unmodified
kernels, in the same process. INT8 K + INT4 V, fp16:
  * Llama-3-8B layer shape (32 query / 8 kv heads, head_dim 128), batch 8 x 16 K tokens: the shape of
    bench.py --workload llama3_8b_decode_attn_seq16k_b8;
  * gpt-oss layer shape (64 query / 8 kv heads, head_dim 64), batch 8 x 16 K tokens, without a window and with window 128.
Wall time per call from events around 50 back-to-back calls (host ctypes / validation included), the median of 15 such
batches is one run; six runs per variant, the variants alternated inside every run. One JSON line per (shape, variant):
the six runs, their range and median, and for the modified variants whether the median lies inside the baseline's range.
Run on the GPU."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

SHAPES = [  # name, B, Hq, Hkv, D, T, window
    ("llama3-8b layer, batch 8 x 16 K", 8, 32, 8, 128, 16384, 0),
    ("gpt-oss layer, batch 8 x 16 K", 8, 64, 8, 64, 16384, 0),
    ("gpt-oss layer, batch 8 x 16 K, window 128", 8, 64, 8, 64, 16384, 128),
]
VARIANTS = [("off", 0.0, False), ("cap", 30.0, False), ("sinks", 0.0, True), ("both", 30.0, True)]


def _batch_us(fn, batches=15, calls=50):
    out = []
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(batches):
        s.record()
        for _ in range(calls):
            fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) * 1e3 / calls)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    from efficient_llm_inference_amd import _lib, kernels as K
    assert torch.cuda.is_available(), "needs the MI355X"
    g = torch.Generator(device="cuda").manual_seed(0)
    lines = []
    for name, B, Hq, Hkv, D, T, W in SHAPES:
        k_store = torch.randint(-127, 128, (B, Hkv, T + 8, D), dtype=torch.int8, device="cuda", generator=g)
        v_store = torch.randint(0, 256, (B, Hkv, T + 8, D // 2), dtype=torch.uint8, device="cuda", generator=g)
        k_sc = torch.rand(T + 8, device="cuda", generator=g) * 0.02 + 0.005
        v_sc = torch.rand(T + 8, device="cuda", generator=g) * 0.02 + 0.005
        q = torch.randn(B, Hq, D, dtype=torch.float16, device="cuda", generator=g)
        kn = torch.randn(B, Hkv, D, dtype=torch.float16, device="cuda", generator=g)
        vn = torch.randn(B, Hkv, D, dtype=torch.float16, device="cuda", generator=g)
        out = torch.empty_like(q)
        sinks = torch.randn(Hq, device="cuda", generator=g)
        ws = torch.empty(K.decode_attn_workspace_cap(B, Hq, Hkv, T + 8, D), dtype=torch.float32, device="cuda")
        plan = K.DecodeStepPlan(q, k_store, k_sc, "int8", v_store, v_sc, "int4", 1e-8)
        fns, logs = {}, {}
        for v, cap, use_sinks in VARIANTS:
            def fn(cap=cap, s=sinks if use_sinks else None):
                K.decode_step(plan, q, kn, vn, T, out, ws, D ** -0.5, window=W, softcap=cap, sinks=s)
            _lib.kernel_log_clear()
            for _ in range(20):  # warm-up of every variant before anything is timed
                fn()
            torch.cuda.synchronize()
            fns[v], logs[v] = fn, _lib.kernel_log()
        runs = {v: [] for v, _, _ in VARIANTS}
        for _ in range(args.runs):
            for v, _, _ in VARIANTS:  # alternated inside every run
                runs[v].append(_batch_us(fns[v]))
        base = runs["off"]
        for v, _, _ in VARIANTS:
            r = runs[v]
            line = dict(shape=name, B=B, Hq=Hq, Hkv=Hkv, D=D, T=T, window=W, variant=v, kernels=logs[v],
                        runs_us=[round(x, 2) for x in r], min_us=round(min(r), 2), max_us=round(max(r), 2),
                        median_us=round(statistics.median(r), 2))
            if v != "off":
                line["baseline_range_us"] = [round(min(base), 2), round(max(base), 2)]
                line["median_inside_baseline_range"] = min(base) <= statistics.median(r) <= max(base)
                line["median_minus_baseline_median_us"] = round(statistics.median(r) - statistics.median(base), 2)
            lines.append(line)
            print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
