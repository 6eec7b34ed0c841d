#!/usr/bin/env python3
"""Attention mass per stored key: kvq_key_scores against the route a caller had before it, alternating in ONE process.

Workload: one layer of Llama-3-8B's store (32 query heads, 8 kv heads, head_dim 128), INT8 keys, fp16 queries, at two shapes:

  snapkv    B 1, T 32,768, S 64   the last 64 prompt queries over the whole prompt
  h2o_step  B 8, T 16,384, S 1    one decode step's queries, after the token was appended

  a  dequant_matmul_softmax   dequantise K to fp16 (kvq_dequant_i8_tokens), then matmul -> fp32 softmax under the causal mask ->
                              sum over the query rows in torch: only operations older than kvq_key_scores, so the same script
                              times a tree without it
  b  key_scores               kernels.key_scores: pass 1, the split merge, pass 2

Each op is timed with HIP events around the whole call after a synchronise, `--reps` times, the ops alternating inside every
repetition; (b)'s first launch (pass 1) is also timed alone through HIP events bound to its dispatch. The record holds the sorted
times, the algorithmic bytes of (b) (K codes twice + scales twice + mass once), bytes / median time as a fraction of 8 TB/s, the
kernels the library launched and the largest difference between the two routes' results. Then `compress_prompt` of the whole
32-layer cache at the snapkv shape (budget 4,096, prefix 4, pool 7). One JSON line per record, then a summary."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

HBM_PEAK = 8e12
SHAPES = {"snapkv": dict(B=1, T=32768, S=64), "h2o_step": dict(B=8, T=16384, S=1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32, help="layers of the cache compress_prompt runs on")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    import efficient_llm_inference_amd as E
    from bench import _time_launches
    from efficient_llm_inference_amd import _lib, kernels
    assert torch.cuda.is_available(), "needs the GPU: a timing from anywhere else says nothing"
    dev = torch.device("cuda:0")
    Hq, Hkv, D = 32, 8, 128
    nq = Hq // Hkv
    sm = D ** -0.5
    lines = []

    def events():
        return [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    for shape, dims in SHAPES.items():
        B, T, S = dims["B"], dims["T"], dims["S"]
        L = a.layers if shape == "snapkv" else 1
        torch.manual_seed(42)
        qc = E.QuantizedKVCache(L, "mixed", device="cuda", compute_dtype=torch.float16)
        qc.reserve(T)
        for l0 in range(0, L, 4):  # a few layers of fp16 at a time
            n = min(4, L - l0)
            past = [(torch.randn(B, Hkv, T, D, device=dev, dtype=torch.float16), torch.randn(B, Hkv, T, D, device=dev, dtype=torch.float16))
                    for _ in range(n)]
            qc._k.append([k for k, _ in past], l0)
            qc._v.append([v for _, v in past], l0)
            del past
        torch.cuda.empty_cache()
        q = torch.randn(B, S, Hq, D, device=dev, dtype=torch.float16).transpose(1, 2)  # HF's projection layout
        k_store, k_sc = qc._k.q[0], qc._k.scales[0]
        ws = torch.empty(kernels.key_scores_workspace(B, Hq, Hkv, T, S, D), device=dev)
        mass = torch.empty(B, Hkv, T, device=dev)
        future = torch.arange(T, device=dev)[None, :] > (T - S + torch.arange(S, device=dev))[:, None]  # [S,T]
        future = future[:, None, :].expand(S, nq, T).transpose(0, 1).reshape(nq * S, T) if S > 1 else None

        def route_a():
            kd = torch.empty(1, B, Hkv, T, D, device=dev, dtype=torch.float16)
            kernels.dequant_tokens(qc._k.q[0:1, :, :, :T], qc._k.scales[0:1, :T], kd, "int8")
            sc = torch.matmul(q.reshape(B, Hkv, nq * S, D), kd[0].transpose(2, 3)).float() * sm  # rows (h, s) of a kv head
            if future is not None:
                sc = sc.masked_fill(future, float("-inf"))
            return torch.softmax(sc, dim=-1).sum(dim=2)

        def route_b():
            kernels.key_scores(q, k_store, k_sc, "int8", T, mass, ws, sm)
            return mass

        ops = {"dequant_matmul_softmax": route_a, "key_scores": route_b}
        times, logs, res = {k: [] for k in ops}, {}, {}
        for rep in range(a.reps + 1):  # repetition 0 warms every shape up
            for name, fn in ops.items():
                torch.cuda.synchronize()
                _lib.kernel_log_clear()
                ev = events()
                ev[0].record()
                out = fn()
                ev[1].record()
                torch.cuda.synchronize()
                logs[name] = _lib.kernel_log()
                res[name] = out.clone()
                del out
                if rep:
                    times[name].append(ev[0].elapsed_time(ev[1]))
        diff = float((res["dequant_matmul_softmax"] - res["key_scores"]).abs().max())
        nbytes = 2 * (B * Hkv * T * D + 4 * T) + 4 * B * Hkv * T
        for name in ops:
            ms = sorted(times[name])
            med = ms[len(ms) // 2]
            rec = {"shape": shape, "op": name, "B": B, "T": T, "S": S, "Hq": Hq, "Hkv": Hkv, "D": D, "ms": [round(x, 4) for x in ms],
                   "median_ms": round(med, 4), "kernels": logs[name],
                   "timer": "HIP events around the whole call (allocations and every launch), synchronised before and after"}
            if name == "key_scores":
                rec.update(algorithmic_bytes=int(nbytes), GBps=round(nbytes / (med * 1e-3) / 1e9, 1),
                           frac_of_8TBps=round(nbytes / (med * 1e-3) / HBM_PEAK, 4), max_abs_diff_to_route_a=diff,
                           mass_sum_over_expected=float(res[name].sum() / (B * Hq * S)))
            lines.append(rec)
        p1 = _time_launches(lambda i: route_b(), a.reps, warm=1)
        lines.append({"shape": shape, "op": "key_scores_pass1_only", "ms": [round(x, 4) for x in p1], "median_ms": round(p1[len(p1) // 2], 4),
                      "kernel": logs["key_scores"][0], "timer": "HIP events bound to the first launch's own dispatch (kvq_time_next_launch)"})
        if shape == "snapkv":  # SnapKV on the whole cache: out of place, so the original tensors are intact
            orig = [(st, st.q, st.scales) for st in (qc._k, qc._v)]
            obs = [torch.randn(B, S, Hq, D, device=dev, dtype=torch.float16).transpose(1, 2) for _ in range(L)]
            cp = []
            kept = None
            for rep in range(a.reps + 1):
                for st, sq, ss in orig:
                    st.q, st.scales = sq, ss
                    st.lens[:] = [T] * L
                    st.staged = 0
                qc._after_eviction()
                torch.cuda.synchronize()
                _lib.kernel_log_clear()
                ev = events()
                ev[0].record()
                keep = qc.compress_prompt(obs, budget=4096, prefix_len=4, pool=7)
                ev[1].record()
                torch.cuda.synchronize()
                kept = int(keep.numel())
                if rep:
                    cp.append(ev[0].elapsed_time(ev[1]))
                torch.cuda.empty_cache()
            cp.sort()
            lines.append({"shape": shape, "op": "compress_prompt", "layers": L, "T": T, "S": S, "budget": 4096, "kept_tokens": kept,
                          "ms": [round(x, 3) for x in cp], "median_ms": round(cp[len(cp) // 2], 3), "kernels": _lib.kernel_log(),
                          "timer": "HIP events around the whole call (every layer's key_scores, the policy, the gather of K and V)"})
        del qc
        torch.cuda.empty_cache()
    med = {(l["shape"], l["op"]): l["median_ms"] for l in lines}
    lines.append({"summary": {s: {"route_a_over_key_scores": round(med[(s, "dequant_matmul_softmax")] / med[(s, "key_scores")], 2),
                                  "condition_b_le_a": med[(s, "key_scores")] <= med[(s, "dequant_matmul_softmax")]} for s in SHAPES}})
    for l in lines:
        print(json.dumps(l), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for l in lines:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
