#!/usr/bin/env python3
"""Left-padded batches (kv_start) in attention over the quantised store: per-layer-call time of the padded kernels against
the unpadded calls they extend. Llama-3-8B layer shape (32 query / 8 kv heads, head_dim 128), INT8 K + INT4 V:
  * batch 8 at T = 16384 and batch 64 at T = 2048: host-count decode (kvq_decode_step) and device-count decode
    (kvq_decode_step_dev) unpadded, then padded with all-zero starts and with starts uniform in [0, T / 2];
  * extend at batch 4, T = 16384, S = 512: unpadded, unpadded under a window that just cuts (W = T + S - 1:
    extend_attn_window_k, the kernel the padded one is a copy of), all-zero starts, starts uniform in [0, T / 2].
Two measures per row, one JSON line each:
  * default: wall time per call from events around 50 back-to-back calls (host ctypes / validation included);
  * --rocprof: kernel time per call. Every row runs in a fresh child process under `rocprofv3 --kernel-trace --stats`
    (tracing only, no counters), and the row's figure is the sum over its kvq kernels of (total duration / launches).
Padded rows also report the share of 8 TB/s computed from the store bytes of the rows actually VISIBLE (named as that).
Runs on a tree without the padded entry points too (the unpadded rows only): the before / after comparison. `--tag` labels
the tree in every line. Run on the GPU."""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

Hq, Hkv, D = 32, 8, 128
ROW_BYTES = D + D // 2  # INT8 K + INT4 V per token and kv head
DECODE = [(8, 16384), (64, 2048)]
EXT = (4, 16384, 512)


def _wall_us(fn, reps):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    out = []
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(reps):
        s.record()
        for _ in range(50):
            fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) * 1e3 / 50)
    return statistics.median(out), min(out), max(out)


def row_names():
    rows = []
    for B, T in DECODE:
        for route in ("host-count", "device-count"):
            for pad in ("unpadded", "kv_start=0", "kv_start~U[0,T/2]"):
                rows.append(f"B={B} T={T} {route} decode {pad}")
    B, T, S = EXT
    for pad in ("unpadded", "window=T+S-1 unpadded", "kv_start=0", "kv_start~U[0,T/2]"):
        rows.append(f"B={B} T={T} S={S} extend {pad}")
    return rows


def rocprof_rows(rows, tag):
    for name in rows:
        d = tempfile.mkdtemp(prefix="psweep_")
        try:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--",
                   sys.executable, os.path.abspath(__file__), "--row", name, "--reps", "3"]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise RuntimeError(f"{name}: rocprofv3 exit {r.returncode}\n{r.stderr[-2000:]}")
            lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
            if not lines:
                print(json.dumps({"row": name, "tree": tag, "skipped": "not on this tree"}), flush=True)
                continue
            stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
            kern = {}
            with open(stats[0]) as f:
                for rec in csv.DictReader(f):
                    if "kvq::" in rec["Name"]:
                        kern[rec["Name"].split("(")[0].replace("void ", "").replace("kvq::", "")] = \
                            (int(rec["Calls"]), float(rec["TotalDurationNs"]) / int(rec["Calls"]) / 1e3)
            us = sum(v[1] for v in kern.values())
            rec = {"row": name, "tree": tag, "kernel_us_per_call": round(us, 2),
                   "kernels": {k: {"calls": c, "us": round(t, 2)} for k, (c, t) in kern.items()}}
            vis = lines[0].get("visible_store_bytes")
            if vis:
                rec["visible_store_bytes"] = vis
                rec["share_of_8TBps_from_visible_rows"] = round(vis / (us * 1e-6) / 8e12, 3)
            print(json.dumps(rec), flush=True)
        finally:
            shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--only", default="", help="comma list of substrings of row names")
    ap.add_argument("--row", default="", help="run this one row only (exact name)")
    ap.add_argument("--rocprof", action="store_true", help="kernel time per call, each row under rocprofv3 (see above)")
    ap.add_argument("--tag", default="", help="label of the tree in every line")
    args = ap.parse_args()
    want = [r for r in row_names() if (not args.only or any(k in r for k in args.only.split(","))) and (not args.row or r == args.row)]
    if args.rocprof:
        rocprof_rows(want, args.tag)
        return
    from efficient_llm_inference_amd import _lib
    from efficient_llm_inference_amd import kernels as K
    dev = torch.device("cuda:0")
    sm = D ** -0.5
    padded = hasattr(_lib.load(), "kvq_decode_attn_padded")

    def store(B, cap):
        g = torch.Generator(device=dev).manual_seed(B)
        ks = torch.randint(-127, 127, (B, Hkv, cap, D), device=dev, dtype=torch.int8, generator=g)
        vs = torch.randint(0, 255, (B, Hkv, cap, D // 2), device=dev, dtype=torch.uint8, generator=g)
        ksc = torch.rand(cap, device=dev, generator=g) * 0.01 + 0.001
        vsc = torch.rand(cap, device=dev, generator=g) * 0.01 + 0.001
        return ks, vs, ksc, vsc

    def starts(B, T, pad):
        if pad == "unpadded":
            return None
        if pad == "kv_start=0":
            return torch.zeros(B, dtype=torch.int32, device=dev)
        return torch.from_numpy(__import__("numpy").random.default_rng(B).integers(0, T // 2 + 1, B).astype("int32")).to(dev)

    def emit(name, fn, B, T, ks):
        _lib.kernel_log_clear()
        fn()
        torch.cuda.synchronize()
        kern = [k.split("(")[0] for k in _lib.kernel_log()]
        med, lo, hi = _wall_us(fn, args.reps)
        vis = int(sum(T - int(s) for s in (ks.tolist() if ks is not None else [0] * B)) * Hkv * ROW_BYTES)
        print(json.dumps({"row": name, "tree": args.tag, "us_per_call": round(med, 2), "us_min": round(lo, 2), "us_max": round(hi, 2),
                          "visible_store_bytes": vis, "share_of_8TBps_from_visible_rows_wall": round(vis / (med * 1e-6) / 8e12, 3),
                          "kernels": kern}), flush=True)

    for name in want:
        pad = name.rsplit(" ", 1)[1]
        if pad != "unpadded" and not padded:
            continue
        kw = {}
        if "extend" in name:
            B, T, S = EXT
            ksv, vsv, ksc, vsc = store(B, T + 8)
            q = torch.randn(B, Hq, S, D, device=dev, dtype=torch.float16)
            kn = torch.randn(B, Hkv, S, D, device=dev, dtype=torch.float16)
            vn = torch.randn_like(kn)
            out = torch.empty_like(q)
            ws = torch.empty(max(1, K.extend_attn_workspace(B, Hq, Hkv, T, S, D)), device=dev, dtype=torch.float32)
            st = starts(B, T, pad)
            if st is not None:
                kw = {"kv_start": st}
            if "window=" in name:
                if not hasattr(_lib.load(), "kvq_extend_attn_window"):
                    continue
                kw = {"window": T + S - 1}
            emit(name, lambda: K.extend_attn(q, ksv, ksc, "int8", vsv, vsc, "int4", T, kn, vn, out, ws, sm, **kw), B, T, st)
            continue
        B = int(name.split()[0][2:])
        T = int(name.split()[1][2:])
        cap = T + 8
        ksv, vsv, ksc, vsc = store(B, cap)
        q = torch.randn(B, Hq, D, device=dev, dtype=torch.float16)
        kn = torch.randn(B, Hkv, D, device=dev, dtype=torch.float16)
        vn = torch.randn_like(kn)
        out = torch.empty_like(q)
        ws = torch.empty(K.decode_attn_workspace_cap(B, Hq, Hkv, cap, D), device=dev, dtype=torch.float32)
        plan = K.DecodeStepPlan(q, ksv, ksc, "int8", vsv, vsc, "int4", 1e-8)
        t_dev = torch.full((1,), T - 1, dtype=torch.int32, device=dev)
        st = starts(B, T - 1, pad)
        if st is not None:
            kw = {"kv_start": st}
        if "host-count" in name:
            emit(name, lambda: K.decode_step(plan, q, kn, vn, T - 1, out, ws, sm, **kw), B, T - 1, st)
        else:
            emit(name, lambda: K.decode_step_dev(plan, q, kn, vn, t_dev, T - 1, out, ws, sm, **kw), B, T - 1, st)


if __name__ == "__main__":
    main()
