"""The float64 model of attention over the quantised store that the tests compare against (numpy, CPU): one function for the
causal mask, HF's sliding window, a left-padded batch's per-row key start and the two score modifiers of the
``kvq_*_ex`` calls, with the helpers that turn a store or a ``tests/attn_cases.Case`` into its arguments.

A query of batch row ``b`` at absolute position ``p`` sees key ``k`` iff ``max(start_b, p - W + 1 if W else 0) <= k <= p``
(W = HF's ``sliding_window``, 0 = none; starts clamped to ``[0, N]``, N keys, as the kernels clamp them). A soft cap c > 0
turns every scaled score s into ``c * tanh(s / c)`` BEFORE masking; a sink is one more softmax term per query head WITHOUT a
value row; a row that sees no key gives zeros (with a sink by arithmetic). The weights are normalised first and then
multiplied by V, the order of ``oracle.kvq_oracle.decode_attention`` / ``extend_attention``: without starts and modifiers the
result equals the oracle's bit for bit (tests/test_attn_ref.py).

``tests/attn_cases.attend`` is not this model: it computes with the exact code x scale values, injects deliberate mistakes
and returns the error budget's terms."""
import numpy as np

from oracle import kvq_oracle as O
from tests.attn_cases import widen


def dequant(k_q, scales_f32, kind, D, kv_dtype="f16"):
    """[B,Hkv,T,Dq] codes + [T] scales -> float64 [B,Hkv,T,D] as the reference's to_past_key_values gives them."""
    if k_q.shape[2] == 0:
        return np.zeros(k_q.shape[:3] + (D,), np.float64)
    d = O.dequantize_tokens(k_q[None], np.asarray(scales_f32, np.float32)[None], kind, D, kv_dtype)[0]
    if kv_dtype == "bf16":
        d = O.bf16_bits_to_f32(d)
    return d.astype(np.float64)


def cap(s, softcap):
    return softcap * np.tanh(s / softcap) if softcap else s


def attention(q, kd, vd, qpos, sm_scale, window=0, kv_start=None, softcap=0.0, sinks=None):
    """q [B,Hq,S,D]; kd / vd [B,Hkv,N,D] float64 keys / values at positions 0..N-1; qpos [S] the queries' positions;
    kv_start None or [B]; sinks None or [Hq]. Returns float64 [B,Hq,S,D]; rows without a visible key are zeros."""
    q = np.asarray(q, np.float64)
    B, Hq, S, D = q.shape
    N = kd.shape[2]
    rep = Hq // kd.shape[1]
    kpos = np.arange(N)[None, :]
    p = np.asarray(qpos)[:, None]
    band = kpos <= p
    if window:
        band = band & (kpos > p - window)
    out = np.zeros((B, Hq, S, D), np.float64)
    for b in range(B):
        vis = band if kv_start is None else band & (kpos >= min(max(int(kv_start[b]), 0), N))
        live = vis.any(axis=1)
        if not live.any():
            continue
        for h in range(Hq):
            s = cap(q[b, h] @ kd[b, h // rep].T * float(sm_scale), softcap)
            s[~vis] = -np.inf
            m = np.where(live, s.max(axis=1), 0.0)[:, None]
            if sinks is not None:
                m = np.maximum(np.where(live[:, None], m, -np.inf), float(sinks[h]))
            e = np.exp(s - m)
            l = e.sum(axis=1, keepdims=True)
            if sinks is not None:
                l = l + np.exp(float(sinks[h]) - m)
            o = (e / np.where(l > 0, l, 1.0)) @ vd[b, h // rep]
            out[b, h] = np.where(live[:, None], o, 0.0)
    return out


def decode(kd, vd, q, kn, vn, T, W, sm_scale, kv_start=None, softcap=0.0, sinks=None):
    """Decode: q [B,Hq,D] at position T (kn / vn [B,Hkv,D] given: the new token, always visible) or T - 1 (kn None) over the
    dequantised stored tokens kd / vd [B,Hkv,>=T,D]. Starts are clamped to the stored count T. Returns [B,Hq,D]."""
    kd, vd = kd[:, :, :T], vd[:, :, :T]
    if kv_start is not None:
        kv_start = np.clip(np.asarray(kv_start, np.int64), 0, T)
    if kn is not None:
        kd = np.concatenate([kd, np.asarray(kn, np.float64)[:, :, None]], axis=2)
        vd = np.concatenate([vd, np.asarray(vn, np.float64)[:, :, None]], axis=2)
    pos = T if kn is not None else T - 1
    return attention(np.asarray(q, np.float64)[:, :, None], kd, vd, [pos], sm_scale, W, kv_start, softcap, sinks)[:, :, 0]


def extend(kd, vd, q, kn, vn, T, W, sm_scale, kv_start=None, softcap=0.0, sinks=None):
    """Extend: q [B,Hq,S,D], chunk kn / vn [B,Hkv,S,D], row s at position T + s. Returns [B,Hq,S,D]."""
    kd = np.concatenate([kd[:, :, :T], np.asarray(kn, np.float64)], axis=2)
    vd = np.concatenate([vd[:, :, :T], np.asarray(vn, np.float64)], axis=2)
    return attention(q, kd, vd, T + np.arange(q.shape[2]), sm_scale, W, kv_start, softcap, sinks)


def decode_lo(T, W, has_new=True):
    """First stored token a decode query sees (at position T with a new token, T - 1 without)."""
    return max(0, T + (1 if has_new else 0) - W) if W else 0


# ---------------------------------------------------------------------------------------- a tests/attn_cases.Case

def keys_values(c, exact=False):
    """Every key and value a query of case ``c`` can see, float64 [B,Hkv,T + Sn,D]: the stored tokens as the reference
    pipeline dequantises them (rounded to the compute dtype; ``exact``: code x scale) followed by the exact new token(s)."""
    if exact:
        kd, vd = c.kint * c.ks.astype(np.float64)[:, None], c.vint * c.vs.astype(np.float64)[:, None]
    else:
        kd, vd = dequant(c.kq, c.ks, c.kinds[0], c.D, c.dtype), dequant(c.vq, c.vs, c.kinds[1], c.D, c.dtype)
    if c.kn is not None:
        kn, vn = widen(c.kn, c.dtype), widen(c.vn, c.dtype)
        if c.mode == "decode":
            kn, vn = kn[:, :, None], vn[:, :, None]
        kd, vd = np.concatenate([kd, kn], axis=2), np.concatenate([vd, vn], axis=2)
    return kd, vd


def positions(c):
    """[S]: the positions of case ``c``'s query rows (extend T + s; decode the last key's)"""
    N = c.T + (0 if c.kn is None else (c.S if c.mode == "extend" else 1))
    return c.T + np.arange(c.S) if c.mode == "extend" else np.array([N - 1])


def visible(c):
    """bool [B,S,N]: the keys each query row of case ``c`` sees (causal, the window's band, the batch row's start)"""
    pos = positions(c)
    kpos = np.arange(pos[-1] + 1)[None, :]
    vis = kpos <= pos[:, None]
    if c.window:
        vis = vis & (kpos > pos[:, None] - c.window)
    vis = np.broadcast_to(vis, (c.B,) + vis.shape).copy()
    if c.kv_start is not None:
        for b, st in enumerate(c.kv_start):
            vis[b] &= kpos >= st
    return vis


def of_case(c, softcap=0.0, sinks=None, exact=False):
    """:func:`attention` of case ``c``: [B,Hq,D] (decode) / [B,Hq,S,D] (extend)"""
    kd, vd = keys_values(c, exact)
    out = attention(widen(c.q, c.dtype), kd, vd, positions(c), c.sm, c.window, c.kv_start, softcap, sinks)
    return out[:, :, 0] if c.mode == "decode" else out
