"""Inputs for attention over the quantised store with the two score modifiers of the ``kvq_*_ex`` calls: logit
soft-capping (Gemma 2) and per-head attention sinks (gpt-oss), and the deliberate mistakes a kernel could make with them. Built
on the arrays of ``tests/attn_cases.Case``; the float64 reference itself is tests/attn_ref.py. Shared by tests/test_attn_mod_discrimination.py (CPU: the check rejects each deliberate mistake on
these inputs) and tests/test_gpu_attn_mod.py (GPU: the kernels pass it).

Semantics (transformers' ``eager_attention_forward`` of the two models):
  soft cap c > 0   every scaled score s (``sm * q . k``, stored, decode's new token and extend's chunk tokens alike) becomes
                   ``c * tanh(s / c)``, BEFORE masking and softmax
  sinks [Hq]       one more softmax term per query head WITHOUT a value row: ``M = max(M, sink[h])``,
                   ``l += exp(sink[h] - M)``; a row that sees no key is zeros (with a sink by arithmetic)

Soft-cap inputs (:func:`make_mod_case`): per (batch row, kv head) the queries of the group lie along one unit direction e with
gain 4 g_h, g_h in [1, 1.5]; every fifth key (and decode's new token, every third chunk token) is ``+-B e`` with
``sm * 4 * B`` in [14, 28], so its score has ``|s| >= 2 c`` for c = 5 (alternating sign, unequal sizes: the uncapped softmax
is owned by the largest positive one, the capped one spreads over all of them at s = c); the other keys are noise with
``|s| < c / 4``.
:func:`score_shares` measures both shares on the dequantised scores, the test asserts them.
Sink inputs (:func:`make_sinks`), per head h by ``h % 4``: 0 a sink 3 above every score batch row 0 sees (M is the sink),
1 a sink EQUAL to that top score, 2 a sink of -1e30 (no effect), 3 a sink at the row's log-sum-exp (half the mass)."""
import numpy as np

from tests import attn_cases as A
from tests import attn_ref
from tests.attn_ref import cap as _cap, keys_values as _keys_values, visible as _visible

CAP = 5.0  # the soft cap the cases are built for
SINK_AMP = 0.2  # make_mod_case(amp=...) of the cases that run with sinks alone
MISTAKES = ("cap_skip_new", "cap_after_max", "cap_before_scale", "sink_by_kv_head", "sink_not_in_max", "sink_value_row",
            "sink_per_split")


def make_mod_case(mode, B, Hq, Hkv, T, S, D, kinds, dtype, seed=0, with_new=True, window=0, kv_start=None, amp=1.0):
    """A :class:`attn_cases.Case` with the soft-cap inputs of the module docstring. ``amp``: the big keys' size relative to that
    (SINK_AMP for a case that runs WITHOUT a cap: its scores then stay below 9, inside what the standard tolerance covers
    when the reference rounds the dequantised keys to the compute dtype and the kernels do not)."""
    rng = np.random.default_rng(seed)
    nq = Hq // Hkv
    Sq = S if mode == "extend" else 1
    Sn = S if mode == "extend" else (1 if with_new else 0)
    sm = D ** -0.5
    Bamp = amp * 3.5 / sm  # amp = 1: sm * 4 * Bamp = 14 >= 2 CAP + margin
    e = rng.choice([-1.0, 1.0], size=(B, Hkv, D)) / np.sqrt(D)  # unit direction per (batch row, kv head)
    gain = rng.uniform(1.0, 1.5, size=(B, Hq, Sq))
    q = 4.0 * gain[..., None] * np.repeat(e, nq, axis=1)[:, :, None, :] + 0.05 * rng.standard_normal((B, Hq, Sq, D))
    k = 0.3 * rng.standard_normal((B, Hkv, T + Sn, D))
    v = rng.standard_normal((B, Hkv, T + Sn, D))
    big = np.zeros(T + Sn, bool)
    big[np.arange(2, T, 5)] = True
    if mode == "extend":
        big[T + np.arange(0, Sn, 3)] = True
    elif Sn:
        big[T] = True
    sign = np.where(np.arange(T + Sn) % 2 == 0, 1.0, -1.0)
    idx = np.nonzero(big)[0]
    amp = Bamp * rng.uniform(1.0, 2.0, size=len(idx))  # unequal: the uncapped softmax is peaked, the capped one is not
    k[:, :, idx] = (sign[idx] * amp)[None, None, :, None] * e[:, :, None, :] + 0.02 * rng.standard_normal((B, Hkv, len(idx), D))
    k_all, v_all, qn = A.narrow(k, dtype), A.narrow(v, dtype), A.narrow(q, dtype)
    if mode == "extend":
        kn, vn = k_all[:, :, T:], v_all[:, :, T:]
    elif Sn:
        kn, vn = k_all[:, :, T], v_all[:, :, T]
    else:
        kn = vn = None
    info = dict(family="mod", variant=None, factor=None, big=big, window=window)
    c = np.ascontiguousarray
    return A.Case(mode, dtype, kinds, sm, qn, c(k_all[:, :, :T]), c(v_all[:, :, :T]), None if kn is None else c(kn),
                  None if vn is None else c(vn), info, window=window, kv_start=kv_start)


def scores(c, softcap=0.0):
    """float64 [B,Hq,S,N] scaled (and capped) scores, before masking"""
    kd, _ = _keys_values(c)
    nq = c.Hq // c.Hkv
    qf = A.widen(c.q, c.dtype)
    return _cap(np.einsum("bhsd,bhnd->bhsn", qf, np.repeat(kd, nq, axis=1)) * c.sm, softcap)


def score_shares(c, cap=CAP):
    """(share of visible keys with |s| >= 2 cap, share with |s| < cap / 4, share in between) over every query row"""
    s = np.abs(scores(c))
    vis = np.broadcast_to(_visible(c)[:, None], s.shape)
    n = vis.sum()
    return ((s >= 2 * cap) & vis).sum() / n, ((s < cap / 4) & vis).sum() / n, ((s >= cap / 4) & (s < 2 * cap) & vis).sum() / n


def make_sinks(c, softcap=0.0):
    """float32 [Hq]: the four sink kinds of the module docstring, from the (capped) scores batch row 0's LAST query row sees"""
    s = scores(c, softcap)[0, :, -1]  # [Hq,N]
    vis = _visible(c)[0, -1]
    out = np.empty(c.Hq, np.float32)
    for h in range(c.Hq):
        sv = s[h][vis]
        top = sv.max() if sv.size else 0.0
        lse = top + np.log(np.exp(sv - top).sum()) if sv.size else 0.0
        out[h] = (top + 3.0, top, -1e30, lse)[h % 4]
    return out


def reference(c, softcap=0.0, sinks=None, mistake=None, splits=2, exact=False):
    """Float64 attention of case ``c`` with the two modifiers: [B,Hq,D] (decode) / [B,Hq,S,D] (extend): tests/attn_ref.py.

    ``mistake``: one deliberate error of a kernel (tests/test_attn_mod_discrimination.py), in a loop of its own:
      cap_skip_new      the cap skipped on the new token / chunk scores only
      cap_after_max     the cap applied after the max subtraction: softmax over cap(s - max s)
      cap_before_scale  the cap applied to q . k before sm_scale
      sink_by_kv_head   the sink indexed by kv head (h // nq) instead of query head
      sink_not_in_max   the sink missing from the max the KEY terms are weighed against: keys e^(s - max s), the sink's own
                        term e^(sink - max(max s, sink)) (with both against the same max the arithmetic would be the same)
      sink_value_row    the sink given a value row (the row's first visible value)
      sink_per_split    the sink added once per split (``splits`` of them) instead of once"""
    if mistake is None:
        return attn_ref.of_case(c, softcap, sinks, exact)
    assert mistake in MISTAKES
    kd, vd = _keys_values(c, exact)
    vis_all = _visible(c)
    nq = c.Hq // c.Hkv
    qf = A.widen(c.q, c.dtype)
    T = c.T
    out = np.zeros((c.B, c.Hq, c.S, c.D))
    for b in range(c.B):
        vis = vis_all[b]
        for h in range(c.Hq):
            g = h // nq
            raw = qf[b, h] @ kd[b, g].T  # [S,N]
            if mistake == "cap_before_scale":
                s = _cap(raw, softcap) * c.sm
            else:
                s = _cap(raw * c.sm, softcap)
            if mistake == "cap_skip_new":
                s[:, T:] = raw[:, T:] * c.sm
            s = np.where(vis, s, -np.inf)
            live = vis.any(axis=1)
            mk = np.where(live, s.max(axis=1), 0.0)[:, None]  # the keys' max
            if mistake == "cap_after_max":
                m0 = np.where(live, np.where(vis, raw * c.sm, -np.inf).max(axis=1), 0.0)[:, None]
                s = np.where(vis, _cap(raw * c.sm - m0, softcap), -np.inf)
                mk = np.where(live, s.max(axis=1), 0.0)[:, None]
            sink = None
            if sinks is not None:
                sink = float(sinks[g if mistake == "sink_by_kv_head" else h])
            M = mk if sink is None else np.maximum(np.where(live[:, None], mk, -np.inf), sink)
            e = np.exp(s - (mk if mistake == "sink_not_in_max" else M))
            l = e.sum(axis=1, keepdims=True)
            o = e @ vd[b, g]
            if sink is not None:
                w = np.exp(sink - M) * (splits if mistake == "sink_per_split" else 1)
                l = l + w
                if mistake == "sink_value_row":
                    first = np.where(live, vis.argmax(axis=1), 0)
                    o = o + w * vd[b, g][first]
            out[b, h] = np.where(l > 0, o / np.where(l > 0, l, 1.0), 0.0)
    return out[:, :, 0] if c.mode == "decode" else out


def tolerance(ref, dtype):
    """The suite's standard tolerance: ``TOL * (|ref| + max |ref|)`` (capped scores are bounded by c: no data-dependent term)"""
    return A.TOL[dtype] * (np.abs(ref) + np.abs(ref).max())


def check(got, ref, dtype):
    """(passes, worst err / tolerance); a non-finite result fails"""
    return A.check(got, ref, tolerance(ref, dtype))
