"""Float64 model of sliding-window attention over the quantised store (HF's ``sliding_window_overlay``: a query at
absolute position p sees key k iff p - W < k <= p; W = 0 means no window), shared by tests/test_sliding_window_host.py
(CPU: it agrees with a brute-force masked softmax) and tests/test_gpu_sliding_window.py (GPU: the kernels match it)."""
import numpy as np

from oracle import kvq_oracle as O


def dequant(k_q, scales_f32, kind, D, kv_dtype="f16"):
    """[B,Hkv,T,Dq] codes + [T] scales -> float64 [B,Hkv,T,D] as the reference's to_past_key_values gives them."""
    if k_q.shape[2] == 0:
        return np.zeros(k_q.shape[:3] + (D,), np.float64)
    d = O.dequantize_tokens(k_q[None], np.asarray(scales_f32, np.float32)[None], kind, D, kv_dtype)[0]
    if kv_dtype == "bf16":
        d = O.bf16_bits_to_f32(d)
    return d.astype(np.float64)


def windowed_attention(q, kd, vd, qpos, W, sm_scale):
    """q [B,Hq,S,D]; kd / vd [B,Hkv,N,D] float64 keys / values at positions 0..N-1; qpos [S] the queries' positions.
    Row s attends keys k with qpos[s] - W < k <= qpos[s] (W = 0: every k <= qpos[s]). Returns float64 [B,Hq,S,D]."""
    q = np.asarray(q, np.float64)
    B, Hq, S, D = q.shape
    N = kd.shape[2]
    rep = Hq // kd.shape[1]
    kpos = np.arange(N)[None, :]
    p = np.asarray(qpos)[:, None]
    vis = kpos <= p
    if W:
        vis &= kpos > p - W
    out = np.empty((B, Hq, S, D), np.float64)
    for b in range(B):
        for h in range(Hq):
            s = q[b, h] @ kd[b, h // rep].T * float(sm_scale)
            s[~vis] = -np.inf
            e = np.exp(s - s.max(axis=1, keepdims=True))
            out[b, h] = (e / e.sum(axis=1, keepdims=True)) @ vd[b, h // rep]
    return out


def decode_lo(T, W, has_new=True):
    """First stored token a decode query sees (at position T with a new token, T - 1 without)."""
    return max(0, T + (1 if has_new else 0) - W) if W else 0
