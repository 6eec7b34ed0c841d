#!/usr/bin/env python3
"""Eviction of a quantised KV store: inside the quantised domain against the fp16 round trip, alternating in ONE process.

Workload: Llama-3-8B's cache (32 layers, batch 1, 8 kv heads, head_dim 128) of 32,768 tokens, mode `mixed` (INT8 K, INT4 V),
chunk summary with chunk 64 / keep 256 and the strided policy with window 256 / stride 4 / prefix 32 (config 5's arguments).

  a  round_trip_chunk_summary   to_past_key_values(copy=True) -> chunk_summarize_kv -> init_from_prompt_past of a new cache:
                                only operations older than the store eviction, so the same script times a tree without it
  b  store_chunk_summarize      QuantizedKVCache.chunk_summarize (kvq_store_chunk_pool, one launch per store)
  c  store_trim_strided         QuantizedKVCache.trim("strided", ...) (kvq_gather_tokens on codes and scale words)
  d  round_trip_strided         to_past_key_values(copy=True) -> trim_kv_strided -> init_from_prompt_past

Each op is timed with HIP events around the whole call (allocations included) after a synchronise, `--reps` times, the ops
alternating inside every repetition; the record holds the sorted times, the algorithmic bytes (computed from the shapes),
bytes / median time as a fraction of 8 TB/s, and the kernels the library launched. One JSON line per op, then a summary."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

HBM_PEAK = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=32768)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    import efficient_llm_inference_amd as E
    from efficient_llm_inference_amd import _lib, cache, kernels
    assert torch.cuda.is_available(), "needs the GPU: a timing from anywhere else says nothing"
    dev = torch.device("cuda:0")
    L, B, H, T, D = a.layers, 1, 8, a.tokens, 128
    chunk, keep = 64, 256
    strided = dict(window_size=256, stride=4, prefix_len=32)
    torch.manual_seed(42)
    past = tuple((torch.randn(B, H, T, D, device=dev, dtype=torch.float16), torch.randn(B, H, T, D, device=dev, dtype=torch.float16))
                 for _ in range(L))
    qc = E.QuantizedKVCache(L, "mixed", device="cuda", compute_dtype=torch.float16)
    qc.init_from_prompt_past(past)
    del past
    torch.cuda.empty_cache()
    orig = [(st, st.q, st.scales) for st in (qc._k, qc._v)]

    def restore():  # the eviction is out of place: the original tensors are intact
        for st, q, s in orig:
            st.q, st.scales = q, s
            st.lens[:] = [T] * L
            st.staged = 0
        qc._attn_plans = {}

    def round_trip(policy):
        new = E.QuantizedKVCache(L, "mixed", device="cuda", compute_dtype=torch.float16)
        new.init_from_prompt_past(policy(qc.to_past_key_values(copy=True)))
        return new._k.lens[0]

    Tout = kernels.chunk_summary_len(T, chunk, keep)
    ops = {"round_trip_chunk_summary": lambda: round_trip(lambda p: E.chunk_summarize_kv(p, chunk, keep)),
           "round_trip_strided": lambda: round_trip(lambda p: cache.trim_kv_strided(p, **strided))}
    if hasattr(qc, "chunk_summarize"):
        ops["store_chunk_summarize"] = lambda: (qc.chunk_summarize(chunk, keep), qc._k.lens[0])[1]
        ops["store_trim_strided"] = lambda: (qc.trim("strided", **strided), qc._k.lens[0])[1]
    code_row = B * H * (D + D // 2)  # bytes of one token's K (INT8) and V (INT4) codes of one layer
    f16_row = B * H * D * 2 * 2      # the same token dequantised, K and V

    def algorithmic_bytes(op, kept):
        if op == "store_chunk_summarize" or op == "store_trim_strided":
            read = T if op == "store_chunk_summarize" else kept
            return L * ((read + kept) * code_row + (read + kept) * 8)
        deq = T * (code_row + 8) + T * f16_row                               # dequantise: codes in, fp16 out
        pol = (T + kept) * f16_row if "chunk" in op else 2 * kept * f16_row  # the fp16 policy
        qnt = kept * f16_row + kept * (code_row + 8)                         # quantise what is left
        return L * (deq + pol + qnt)

    times = {k: [] for k in ops}
    kept_of, logs = {}, {}
    for rep in range(a.reps + 1):  # repetition 0 warms every shape up
        for name, fn in ops.items():
            restore()
            torch.cuda.synchronize()
            _lib.kernel_log_clear()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            kept_of[name] = fn()
            ev[1].record()
            torch.cuda.synchronize()
            logs[name] = _lib.kernel_log()
            if rep:
                times[name].append(ev[0].elapsed_time(ev[1]))
            torch.cuda.empty_cache()
    lines = []
    for name in ops:
        ms = sorted(times[name])
        med = ms[len(ms) // 2]
        nbytes = algorithmic_bytes(name, kept_of[name])
        lines.append({"op": name, "layers": L, "tokens": T, "kept_tokens": kept_of[name], "ms": [round(x, 3) for x in ms], "median_ms": round(med, 3),
                      "algorithmic_bytes": int(nbytes), "GBps": round(nbytes / (med * 1e-3) / 1e9, 1),
                      "frac_of_8TBps": round(nbytes / (med * 1e-3) / HBM_PEAK, 4), "kernels": logs[name],
                      "timer": "HIP events around the whole call (allocations and every launch), synchronised before and after"})
    if hasattr(kernels, "store_chunk_pool"):  # the launch alone: HIP events bound to the kernel's own dispatch
        from bench import _time_launches
        restore()
        for st, label in ((qc._k, "store_pool_kernel_k_int8"), (qc._v, "store_pool_kernel_v_int4")):
            Dq = st.q.size(4)
            q_out = torch.empty(L, B, H, Tout, Dq, dtype=st.q.dtype, device=dev)
            s_out = torch.empty(L, Tout, dtype=torch.float32, device=dev)
            _lib.kernel_log_clear()
            ms = _time_launches(lambda i: kernels.store_chunk_pool(st.q[:, :, :, :T], st.scales[:, :T], q_out, s_out, st.kind, D,
                                                                   torch.float16, chunk, keep), a.reps, warm=1)
            nbytes = L * (T + Tout) * (B * H * Dq + 4)
            med_k = ms[len(ms) // 2]
            lines.append({"op": label, "layers": L, "tokens": T, "kept_tokens": Tout, "ms": [round(x, 4) for x in ms], "median_ms": round(med_k, 4),
                          "algorithmic_bytes": int(nbytes), "GBps": round(nbytes / (med_k * 1e-3) / 1e9, 1),
                          "frac_of_8TBps": round(nbytes / (med_k * 1e-3) / HBM_PEAK, 4), "kernels": _lib.kernel_log(),
                          "timer": "HIP events bound to the launch's own dispatch (kvq_time_next_launch)"})
    med = {l["op"]: l["median_ms"] for l in lines}
    if "store_chunk_summarize" in med:
        lines.append({"summary": {"chunk_summary_round_trip_over_store": round(med["round_trip_chunk_summary"] / med["store_chunk_summarize"], 2),
                                  "strided_round_trip_over_store": round(med["round_trip_strided"] / med["store_trim_strided"], 2),
                                  "expected_kept": {"chunk_summary": Tout}}})
    for l in lines:
        print(json.dumps(l), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
