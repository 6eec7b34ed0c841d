"""Float64 model of attention over the quantised store for a LEFT-PADDED batch, shared by tests/test_padded_host.py (CPU: it
agrees with a brute-force masked softmax) and tests/test_gpu_padded_attn.py (GPU: the padded kernels match it).

``kv_start[b]``: key positions ``k < kv_start[b]`` of batch row ``b`` are padding. A query of row ``b`` at absolute position
``p`` sees key ``k`` iff ``max(kv_start[b], p - W + 1 if W else 0) <= k <= p`` (W = HF's sliding window, 0 = none). A query
that sees no key gives zeros. Starts are clamped to ``[0, N]`` (N keys), as the kernels clamp them."""
import numpy as np

from tests.window_ref import dequant  # noqa: F401  (the store's float64 values, for callers)


def padded_attention(q, kd, vd, qpos, W, sm_scale, kv_start):
    """q [B,Hq,S,D]; kd / vd [B,Hkv,N,D] float64 keys / values at positions 0..N-1; qpos [S] the queries' positions;
    kv_start [B]. Returns float64 [B,Hq,S,D]; rows without a visible key are zeros."""
    q = np.asarray(q, np.float64)
    B, Hq, S, D = q.shape
    N = kd.shape[2]
    rep = Hq // kd.shape[1]
    kpos = np.arange(N)[None, :]
    p = np.asarray(qpos)[:, None]
    band = kpos <= p
    if W:
        band = band & (kpos > p - W)
    out = np.zeros((B, Hq, S, D), np.float64)
    for b in range(B):
        st = min(max(int(kv_start[b]), 0), N)
        vis = band & (kpos >= st)
        live = vis.any(axis=1)
        if not live.any():
            continue
        for h in range(Hq):
            s = q[b, h] @ kd[b, h // rep].T * float(sm_scale)
            s[~vis] = -np.inf
            m = np.where(live, s.max(axis=1), 0.0)[:, None]
            e = np.exp(s - m)
            l = e.sum(axis=1, keepdims=True)
            o = (e / np.where(l > 0, l, 1.0)) @ vd[b, h // rep]
            out[b, h] = np.where(live[:, None], o, 0.0)
    return out


def decode_ref(kd, vd, q, kn, vn, T, W, sm_scale, kv_start):
    """Decode: q [B,Hq,D] at position T (kn / vn [B,Hkv,D] given: the new token, always visible) or T - 1 (kn None) over the
    dequantised stored tokens kd / vd [B,Hkv,>=T,D]. Starts are clamped to the stored count T. Returns [B,Hq,D]."""
    kd, vd = kd[:, :, :T], vd[:, :, :T]
    st = np.clip(np.asarray(kv_start, np.int64), 0, T)
    if kn is not None:
        kd = np.concatenate([kd, np.asarray(kn, np.float64)[:, :, None]], axis=2)
        vd = np.concatenate([vd, np.asarray(vn, np.float64)[:, :, None]], axis=2)
    pos = T if kn is not None else T - 1
    return padded_attention(np.asarray(q, np.float64)[:, :, None], kd, vd, [pos], W, sm_scale, st)[:, :, 0]


def extend_ref(kd, vd, q, kn, vn, T, W, sm_scale, kv_start):
    """Extend: q [B,Hq,S,D], chunk kn / vn [B,Hkv,S,D], row s at position T + s. Returns [B,Hq,S,D]."""
    S = q.shape[2]
    kd = np.concatenate([kd[:, :, :T], np.asarray(kn, np.float64)], axis=2)
    vd = np.concatenate([vd[:, :, :T], np.asarray(vn, np.float64)], axis=2)
    return padded_attention(q, kd, vd, T + np.arange(S), W, sm_scale, kv_start)
