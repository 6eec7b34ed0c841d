#!/usr/bin/env python3
"""Sliding-window attention over the quantised store: per-layer-call time of the windowed kernels against what they
should cost. Llama-3-8B layer shape (32 query / 8 kv heads, head_dim 128), INT8 K + INT4 V, T = 16384:
  * host-count decode (kvq_decode_step_window) at batch 8: no window, W = 4096, and the unwindowed call at T = 4095;
  * device-count decode (kvq_decode_step_dev_window) at batch 8, t_bound = 16383, W = 4096, against the host-count call;
  * extend (kvq_extend_attn_window) at batch 1, S = 512: no window and W = 4096;
  * the unwindowed host-count decode at batch 1 (the calls the device-count change shares kernels with).
Two measures per row, one JSON line each:
  * default: wall time per call from events around 50 back-to-back calls (host ctypes / validation included: sub-40 us
    calls sit near the host floor, so this is NOT the kernel time);
  * --rocprof: kernel time per call. Every row runs in a fresh child process under `rocprofv3 --kernel-trace --stats`,
    and the row's figure is the sum over its kvq kernels of (total duration / launches): the GPU time of one call, no host
    time and no gaps between launches.
Runs on a tree without the windowed entry points too (the unwindowed rows only): the before / after comparison of the
unwindowed rows. Run on the GPU."""
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


def _wall_us(fn, reps):
    """median host-to-host time per call over batches of 50 back-to-back calls (includes every launch of the call)"""
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
    return statistics.median(out)


ROWS = [
    "B=8 host-count decode T=16383 no window",
    "B=8 host-count decode T=4095 no window",
    "B=8 host-count decode T=16383 W=4096",
    "B=8 device-count decode t=16383 bound=16383 W=4096",
    "B=8 device-count decode t=16383 bound=16383 no window",
    "B=1 host-count decode T=16384 no window (decode_attn)",
    "B=1 extend T=16384 S=512 no window",
    "B=1 extend T=16384 S=512 W=4096",
    "B=1 extend T=4095 S=512 no window",
]


def rocprof_rows(rows, reps, tag):
    """each row in its own child process under rocprofv3 kernel statistics: kernel time per call"""
    for name in rows:
        d = tempfile.mkdtemp(prefix="wsweep_")
        try:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--",
                   sys.executable, os.path.abspath(__file__), "--row", name, "--reps", str(reps)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise RuntimeError(f"{name}: rocprofv3 exit {r.returncode}\n{r.stderr[-2000:]}")
            if not any(line.startswith("{") for line in r.stdout.splitlines()):
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
            print(json.dumps({"row": name, "tree": tag, "kernel_us_per_call": round(us, 2),
                              "kernels": {k: {"calls": c, "us": round(t, 2)} for k, (c, t) in kern.items()}}), flush=True)
        finally:
            shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--only", default="", help="comma list of rows: decode, dev, extend, b1")
    ap.add_argument("--row", default="", help="run this one row only (exact name)")
    ap.add_argument("--rocprof", action="store_true", help="kernel time per call, each row under rocprofv3 (see above)")
    ap.add_argument("--tag", default="", help="label of the tree in --rocprof lines")
    args = ap.parse_args()
    if args.rocprof:
        rocprof_rows([r for r in ROWS if not args.only or any(k in r for k in args.only.split(","))], 3, args.tag)
        return
    from efficient_llm_inference_amd import _lib
    from efficient_llm_inference_amd import kernels as K
    dev = torch.device("cuda:0")
    Hq, Hkv, D, T, W = 32, 8, 128, 16384, 4096
    sm = D ** -0.5
    only = set(filter(None, args.only.split(",")))
    win = hasattr(_lib.load(), "kvq_decode_attn_window")

    def store(B, cap):
        g = torch.Generator(device=dev).manual_seed(B)
        ks = torch.randint(-127, 127, (B, Hkv, cap, D), device=dev, dtype=torch.int8, generator=g)
        vs = torch.randint(0, 255, (B, Hkv, cap, D // 2), device=dev, dtype=torch.uint8, generator=g)
        ksc = torch.rand(cap, device=dev, generator=g) * 0.01 + 0.001
        vsc = torch.rand(cap, device=dev, generator=g) * 0.01 + 0.001
        return ks, vs, ksc, vsc

    def row(name, fn):
        if args.row and name != args.row:
            return
        _lib.kernel_log_clear()
        fn()
        torch.cuda.synchronize()
        kern = [k.split("(")[0] for k in _lib.kernel_log()]
        us = _wall_us(fn, args.reps)
        print(json.dumps({"row": name, "us_per_call": round(us, 2), "kernels": kern}), flush=True)

    def decode_rows(B, rows):
        cap = T + 8
        ks, vs, ksc, vsc = store(B, cap)
        q = torch.randn(B, Hq, D, device=dev, dtype=torch.float16)
        kn = torch.randn(B, Hkv, D, device=dev, dtype=torch.float16)
        vn = torch.randn_like(kn)
        out = torch.empty_like(q)
        ws = torch.empty(K.decode_attn_workspace_cap(B, Hq, Hkv, cap, D), device=dev, dtype=torch.float32)
        plan = K.DecodeStepPlan(q, ks, ksc, "int8", vs, vsc, "int4", 1e-8)
        t_dev = torch.full((1,), T - 1, dtype=torch.int32, device=dev)
        for name, fn in rows(plan, q, kn, vn, out, ws, t_dev):
            row(f"B={B} {name}", fn)

    if not only or "decode" in only or "dev" in only:
        def rows(plan, q, kn, vn, out, ws, t_dev):
            r = [("host-count decode T=16383 no window", lambda: K.decode_step(plan, q, kn, vn, T - 1, out, ws, sm)),
                 ("host-count decode T=4095 no window", lambda: K.decode_step(plan, q, kn, vn, W - 1, out, ws, sm))]
            if win:
                r += [("host-count decode T=16383 W=4096", lambda: K.decode_step(plan, q, kn, vn, T - 1, out, ws, sm, window=W)),
                      ("device-count decode t=16383 bound=16383 W=4096",
                       lambda: K.decode_step_dev(plan, q, kn, vn, t_dev, T - 1, out, ws, sm, window=W)),
                      ("device-count decode t=16383 bound=16383 no window",
                       lambda: K.decode_step_dev(plan, q, kn, vn, t_dev, T - 1, out, ws, sm))]
            return r
        decode_rows(8, rows)
    if not only or "b1" in only:
        def rows1(plan, q, kn, vn, out, ws, t_dev):
            return [("host-count decode T=16384 no window (decode_attn)", lambda: K.decode_attn(
                q, plan.keep[0], plan.keep[2], "int8", plan.keep[1], plan.keep[3], "int4", T, out, ws, sm, kn, vn))]
        decode_rows(1, rows1)
    if not only or "extend" in only:
        B, S = 1, 512
        ks, vs, ksc, vsc = store(B, T + 8)
        q = torch.randn(B, Hq, S, D, device=dev, dtype=torch.float16)
        kn = torch.randn(B, Hkv, S, D, device=dev, dtype=torch.float16)
        vn = torch.randn_like(kn)
        out = torch.empty_like(q)
        ws = torch.empty(max(1, K.extend_attn_workspace(B, Hq, Hkv, T, S, D)), device=dev, dtype=torch.float32)
        row("B=1 extend T=16384 S=512 no window",
            lambda: K.extend_attn(q, ks, ksc, "int8", vs, vsc, "int4", T, kn, vn, out, ws, sm))
        if win:
            row("B=1 extend T=16384 S=512 W=4096",
                lambda: K.extend_attn(q, ks, ksc, "int8", vs, vsc, "int4", T, kn, vn, out, ws, sm, window=W))
            row("B=1 extend T=4095 S=512 no window",
                lambda: K.extend_attn(q, ks, ksc, "int8", vs, vsc, "int4", W - 1, kn, vn, out, ws, sm))


if __name__ == "__main__":
    main()
