"""A shadow model of ``QuantizedKVCache``'s life cycle and the scripts that drive it (numpy, CPU only), shared by
tests/test_cache_lifecycle_model.py (CPU: the scripts, the capacity prediction and the driver are self-consistent, and each
deliberate mistake of the stateful layer is rejected) and tests/test_gpu_cache_lifecycle.py (GPU: the real cache passes).

:class:`ShadowCache` restates the cache's surface from what the suite already trusts: ``oracle.kvq_oracle`` for quantise,
dequantise, the keep-index policies and the gather; ``tests.attn_ref`` for attention; ``tests.store_evict_cases.model`` for the
chunk summary; ``tests.key_score_cases`` for the key masses and the top-score rule. Its state is, per store, the codes
``[G,B,H,cap,Dq]``, the scale words ``[G,cap]`` (fp32), ``lens``, ``cap``, the staging buffer with ``staged``, and an
allocation counter that stands for ``data_ptr()``.

A script is a list of ``(op, kwargs)`` tuples whose arrays come from a seed (:func:`build_script`). :func:`run_script` applies
every step to the subject and to a fresh shadow and compares after EVERY step: codes and scale words of ``[0, T)`` bit for bit,
``lens``, ``len(layers[i])``, ``estimated_bytes()``, the predicted capacity against the tensors' own dimensions (it never
shrinks; an eviction keeps it unless the kept list does not fit; a no-op leaves the allocation alone), every attend / extend /
key_scores result against the shadow's state BEFORE the call under the suite's standard tolerance, and at the marked steps the
incremental ``to_past_key_values()`` against ``copy=True`` and the shadow's dequantised state, bit for bit. The first failing
step is named in the :class:`StepFailure`.

Inputs make output-only mistakes visible. Every token written carries a Hadamard direction of its kv head (sign and index
from the token's serial number) and values of its own. A query aims (8 nats: scaled scores stay below 9, the bound
``attn_mod_cases.SINK_AMP`` documents for the standard tolerance) at the most recently written stored token as the store
holds it (the appended token, a token gathered to a new slot, a pooled summary), at the exact new token, and, after an
eviction, at a GHOST: a token that no longer exists, which only a stale store would still answer. Chunk row ``s`` aims at chunk
tokens ``s`` and ``s + 1``: the second must stay unseen.

A subject offers ``init_from_prompt_past, append_from_past, attend, extend, key_scores, evict_by_scores, compress_prompt,
keep_tokens, trim, chunk_summarize, reserve, to_past_key_values, reduce_scores, state, launches`` (the kernel log since the
last call; ``native = True`` on a subject that launches kernels); arrays travel as numpy in the compute dtype's representation
(fp16 arrays, bf16 as uint16 bits), results come back as float64 / float32 numpy."""
import os
import types

import numpy as np

from oracle import kvq_oracle as O
from tests import attn_mod_cases, attn_ref, key_score_cases, store_evict_cases
from tests.attn_cases import TOL, hadamard, narrow, widen

L, B, HKV, HQ = 2, 2, 2, 8
PROMPT = 17
CAPS = (24, 56, 120)  # the capacities a 17-token prompt walks through: asserted literally by the scripts
CONFIGS = (("mixed", "f16", 128), ("int4", "bf16", 64), ("int8", "bf16", 128))
MODE_KINDS = {"int8": ("int8", "int8"), "int4": ("int4", "int4"), "mixed": ("int8", "int4")}
AIM = 8.0  # nats: the scaled score of an aimed-at token
SCRIPTS = ("growth", "evict", "variants", "mid_walk")
VARIANTS = ("window", "kv_start", "softcap", "sinks")
WINDOW = 20  # keys: cuts every store the variants script runs on

# name -> the script that must reject it; the second field says what kind of check does ("bits", "lens", "cap", "alloc",
# "staging": exact; "output": by at least 5x the tolerance)
MISTAKES = {
    "append_lost_on_growth": ("growth", "bits"),
    "stale_tokens_after_eviction": ("evict", "output"),
    "append_to_old_T_after_eviction": ("evict", "bits"),
    "stage_kept_across_eviction": ("evict", "staging"),
    "stage_not_copied_on_growth": ("growth", "staging"),
    "v_lens_not_updated": ("evict", "lens"),
    "scales_not_gathered": ("evict", "bits"),
    "pool_tail_scales_off_by_one": ("evict", "bits"),
    "extend_appends_first": ("growth", "output"),
    "key_scores_prev_T": ("growth", "output"),
    "cap_reset_by_eviction": ("evict", "cap"),
    "noop_trim_reallocates": ("evict", "alloc"),
}


def skewed_capacity(n):
    return (n + 7) // 16 * 16 + 8


def odt(dtype):
    return "bf16" if dtype == "bf16" else None


def packed_dim(kind, D):
    return D if kind == "int8" else (D + 1) // 2


def keep_indices(policy, T, **kw):
    """the oracle's keep-index policies by the cache's policy names (None: keep everything)"""
    if policy == "sliding_window":
        w = kw["window_size"]
        return None if (not T > w or w == 0) else list(range(T - w, T))
    return getattr(O, "keep_indices_" + policy)(T, **kw)


class StepFailure(AssertionError):
    """A script step the subject failed: ``step`` (index), ``op``, ``check`` (bits / lens / cap / alloc / staging / output /
    raises / launches / kept) and, for an output check, ``ratio`` = worst error / tolerance."""

    def __init__(self, script, step, op, check, detail, ratio=None):
        self.script, self.step, self.op, self.check, self.ratio = script, step, op, check, ratio
        super().__init__(f"script {script!r} step {step} ({op}): {check}: {detail}")


# ------------------------------------------------------------------------------------------------------------ the shadow

class _Store:
    def __init__(self, kind, G, dtype, owner):
        self.kind, self.G, self.dtype, self.owner = kind, G, dtype, owner
        self.lens = [0] * G
        self.q = self.s = self.stage = None
        self.cap = self.staged = self.want = self.alloc = 0
        self.B = self.H = self.D = None
        self.pre = None  # (codes, scales, T) before the last eviction: what a stale plan would still read

    def _empty(self, cap):
        qd = np.int8 if self.kind == "int8" else np.uint8
        return np.zeros((self.G, self.B, self.H, cap, packed_dim(self.kind, self.D)), qd), np.zeros((self.G, cap), np.float32)

    def _empty_stage(self, cap):
        return np.zeros((self.G, self.B, self.H, cap, self.D), np.uint16 if self.dtype == "bf16" else np.float16)

    def reserve(self, T):
        if self.B is None or T <= self.cap:
            self.want = max(self.want, T)
            return False
        cap = skewed_capacity(max(T, 2 * self.cap, 16))
        q, s = self._empty(cap)
        used = max(self.lens)
        if self.q is not None and used:
            q[:, :, :, :used] = self.q[:, :, :, :used]
            s[:, :used] = self.s[:, :used]
        self.q, self.s, self.cap = q, s, cap
        self.alloc += 1
        if self.stage is not None:
            st = self._empty_stage(cap)
            if self.staged and self.owner.mistake != "stage_not_copied_on_growth":
                st[:, :, :, :self.staged] = self.stage[:, :, :, :self.staged]
            self.stage = st
        return True

    def bind(self, x):
        if self.B is None:
            self.B, self.H, _, self.D = x.shape
            self.reserve(max(self.want, 1))

    def append(self, xs, g0=0, slot=None, lost=False):
        """xs: one [B,H,Tn,D] array per group g0..; ``slot``: where the tokens go instead of the group's length; ``lost``:
        the tokens are not written at all (the counts still move)"""
        self.bind(xs[0])
        n, Tn = len(xs), xs[0].shape[2]
        t0 = self.lens[g0]
        assert all(self.lens[g0 + i] == t0 for i in range(n))
        self.reserve(t0 + Tn)
        q, _, s = O.quantize_tokens(np.stack(xs), self.kind, dtype=odt(self.dtype))
        at = t0 if slot is None else slot
        if not lost and at + Tn <= self.cap:
            self.q[g0:g0 + n, :, :, at:at + Tn] = q.view(self.q.dtype)
            self.s[g0:g0 + n, at:at + Tn] = s
        for i in range(n):
            self.lens[g0 + i] = t0 + Tn

    def uniform_len(self):
        if any(n != self.lens[0] for n in self.lens):
            raise ValueError("kvq: all groups of a store must hold the same number of tokens")
        return self.lens[0]

    def dequant(self, g, T=None, t0=0):
        """groups g (a slice), tokens [t0, T) in the compute dtype's representation"""
        T = self.lens[g.start if isinstance(g, slice) else g] if T is None else T
        gs = g if isinstance(g, slice) else slice(g, g + 1)
        return O.dequantize_tokens(self.q[gs, :, :, t0:T], self.s[gs, t0:T], self.kind, self.D, self.dtype)

    def _swap(self, q, s, cap, T, move_lens=True):
        m = self.owner.mistake
        self.pre = (self.q, self.s, self.lens[0])
        self.q, self.s = q, s
        self.alloc += 1
        if m == "cap_reset_by_eviction":
            cap = skewed_capacity(T)
            self.q, self.s = q[:, :, :, :cap], s[:, :cap]
        if cap != self.cap:
            self.cap, self.stage = cap, None
        if move_lens:
            self.lens[:] = [T] * self.G
        if m != "stage_kept_across_eviction":
            self.staged = 0

    def _fresh(self, need):
        cap = self.cap if need <= self.cap else skewed_capacity(need)
        return self._empty(cap) + (cap,)

    def gather(self, idx, move_lens=True):
        T, n = self.uniform_len(), len(idx)
        q, s, cap = self._fresh(n)
        ok = np.array([0 <= i < T for i in idx])
        sel = np.where(ok, np.asarray(idx, np.int64), 0)
        q[:, :, :, :n] = np.where(ok[None, None, None, :, None], self.q[:, :, :, sel], 0)
        s[:, :n] = self.s[:, :n] if self.owner.mistake == "scales_not_gathered" else np.where(ok[None], self.s[:, sel], 0)
        self._swap(q, s, cap, n, move_lens)

    def chunk_pool(self, chunk, keep, move_lens=True):
        T = self.uniform_len()
        case = dict(q=self.q[:, :, :, :T], s=self.s[:, :T], kind=self.kind, dtype=self.dtype, D=self.D, chunk=chunk, keep=keep)
        q2, s2 = store_evict_cases.model(case)
        Tout = q2.shape[3]
        k = min(keep, T)
        if self.owner.mistake == "pool_tail_scales_off_by_one" and k:
            s2 = s2.copy()
            s2[:, Tout - k:] = self.s[:, T - k - 1:T - 1]
        q, s, cap = self._fresh(Tout)
        q[:, :, :, :Tout], s[:, :Tout] = q2, s2
        self._swap(q, s, cap, Tout, move_lens)

    def dequant_staged(self):
        T = self.uniform_len()
        if self.stage is None:
            self.stage, self.staged = self._empty_stage(self.cap), 0
        if self.staged < T:
            self.stage[:, :, :, self.staged:T] = self.dequant(slice(0, self.G), T, self.staged)
            self.staged = T
        return self.stage[:, :, :, :T].copy()


class ShadowCache:
    """``QuantizedKVCache(L, mode, compute_dtype=dtype)`` in numpy. ``mistake``: one name of :data:`MISTAKES`, a deliberate
    error of the stateful layer (tests/test_cache_lifecycle_model.py)."""

    def __init__(self, n_layers, mode, dtype, mistake=None):
        assert mistake is None or mistake in MISTAKES, mistake
        self.L, self.mode, self.dtype, self.mistake = n_layers, mode, dtype, mistake
        kk, vk = MODE_KINDS[mode]
        self.k, self.v = _Store(kk, n_layers, dtype, self), _Store(vk, n_layers, dtype, self)
        self.evicted = False  # an eviction has run and no token was appended since

    # -- state ------------------------------------------------------------------------------------------------------
    def state(self):
        k, v = self.k, self.v
        per = lambda st, T: T * (st.B * st.H * packed_dim(st.kind, st.D) + 2) if st.B is not None else 0
        return dict(k=(k.q, k.s), v=(v.q, v.s), klens=list(k.lens), vlens=list(v.lens), kcap=k.cap, vcap=v.cap,
                    alloc=(k.alloc, v.alloc), layer_lens=list(k.lens),
                    bytes=sum(per(k, k.lens[g]) + per(v, v.lens[g]) for g in range(self.L)))

    def launches(self):
        return []

    def reduce_scores(self, table):
        return np.asarray(table, np.float32).reshape(-1, table.shape[-1]).sum(axis=0, dtype=np.float32)

    def dequantised(self):
        """[(K, V)] per layer, every stored token, in the compute dtype's representation"""
        kd, vd = self.k.dequant(slice(0, self.L)), self.v.dequant(slice(0, self.L))
        return [(kd[i], vd[i]) for i in range(self.L)]

    def key_at(self, layer, slot):
        """float64 [B,Hkv,D]: the stored key at ``slot`` as attention sees it"""
        k = self.k
        return attn_ref.dequant(k.q[layer][:, :, slot:slot + 1], k.s[layer][slot:slot + 1], k.kind, k.D, self.dtype)[:, :, 0]

    # -- the cache's surface ------------------------------------------------------------------------------------------
    def reserve(self, n):
        self.k.reserve(n)
        self.v.reserve(n)

    def init_from_prompt_past(self, past):
        self.k.append([k for k, _ in past])
        self.v.append([v for _, v in past])
        self.evicted = False

    def append_from_past(self, past):
        self.k.append([k[:, :, -1:] for k, _ in past])
        self.v.append([v[:, :, -1:] for _, v in past])
        self.evicted = False

    def to_past_key_values(self, copy=False):
        k, v = self.k, self.v
        if len(set(k.lens)) != 1 or len(set(v.lens)) != 1:
            raise ValueError("kvq: groups dequantised together must hold the same number of tokens")
        if k.lens[0] == 0:
            raise ValueError("Empty cache")
        if copy:
            return self.dequantised()
        kd, vd = k.dequant_staged(), v.dequant_staged()
        return [(kd[i], vd[i]) for i in range(self.L)]

    def _kv(self, layer, T, stale=False):
        out = []
        for st in (self.k, self.v):
            q, s = st.q, st.s
            if stale and st.pre is not None:
                q, s, T = st.pre
            out.append(attn_ref.dequant(q[layer][:, :, :T], s[layer][:T], st.kind, st.D, self.dtype))
        return out[0], out[1], T

    def _append_layer(self, layer, kn, vn):
        """kn / vn [B,H,Tn,D] into ``layer``'s groups, with the append mistakes"""
        kw = {}
        if self.mistake == "append_to_old_T_after_eviction" and self.evicted and self.k.pre is not None:
            kw = dict(slot=self.k.pre[2])
        if self.mistake == "append_lost_on_growth" and self.k.lens[layer] + kn.shape[2] > self.k.cap:
            kw = dict(lost=True)
        self.k.append([kn], layer, **kw)
        self.v.append([vn], layer, **kw)
        if layer == self.L - 1:
            self.evicted = False

    def attend(self, layer, q, k_new=None, v_new=None, append=False, window=None, kv_start=None, softcap=0.0, sinks=None):
        T = self.k.lens[layer]
        if T != self.v.lens[layer] or self.k.q is None:
            raise ValueError("Empty cache")
        D = q.shape[-1]
        kd, vd, Ts = self._kv(layer, T, stale=self.mistake == "stale_tokens_after_eviction" and self.evicted)
        kn = None if k_new is None else widen(k_new, self.dtype)
        vn = None if v_new is None else widen(v_new, self.dtype)
        out = attn_ref.decode(kd, vd, widen(q, self.dtype), kn, vn, Ts, window or 0, D ** -0.5, kv_start, softcap, sinks)
        if append:
            self._append_layer(layer, k_new[:, :, None], v_new[:, :, None])
        return out

    def extend(self, layer, q, k_new, v_new, append=True, window=None, kv_start=None, softcap=0.0, sinks=None):
        T = self.k.lens[layer]
        D = q.shape[-1]
        if self.mistake == "extend_appends_first" and append:
            self._append_layer(layer, k_new, v_new)
            kd, vd, Ts = self._kv(layer, self.k.lens[layer])
            return attn_ref.extend(kd, vd, widen(q, self.dtype), widen(k_new, self.dtype), widen(v_new, self.dtype), Ts,
                                   window or 0, D ** -0.5, kv_start, softcap, sinks)
        kd, vd, Ts = self._kv(layer, T, stale=self.mistake == "stale_tokens_after_eviction" and self.evicted)
        out = attn_ref.extend(kd, vd, widen(q, self.dtype), widen(k_new, self.dtype), widen(v_new, self.dtype), Ts,
                              window or 0, D ** -0.5, kv_start, softcap, sinks)
        if append:
            self._append_layer(layer, k_new, v_new)
        return out

    def key_scores(self, layer, q):
        k = self.k
        T = k.lens[layer]
        if T == 0 or k.q is None:
            raise ValueError("Empty cache")
        if q.ndim == 3:
            q = q[:, :, None]
        Tm = T - 1 if (self.mistake == "key_scores_prev_T" and T > q.shape[2]) else T
        kint = key_score_cases.stored_codes(k.q[layer][:, :, :Tm], k.kind, k.D)
        mass = key_score_cases.key_mass_stored(q, kint, k.s[layer][:Tm], self.dtype, k.D ** -0.5)
        return np.concatenate([mass, np.zeros(mass.shape[:2] + (T - Tm,))], axis=2)

    def _evictable_len(self):
        T = self.k.uniform_len()
        if T != self.v.uniform_len():
            raise ValueError("kvq: the K and V stores hold different token counts")
        if T == 0 or self.k.q is None:
            raise ValueError("Empty cache")
        return T

    def keep_tokens(self, idx):
        T = self._evictable_len()
        idx = [int(i) for i in idx]
        if not idx:
            raise ValueError("kvq: keep_tokens needs at least one token")
        if min(idx) < 0 or max(idx) >= T:
            raise ValueError(f"kvq: keep_tokens index out of range [0, {T})")
        self.k.gather(idx)
        self.v.gather(idx, move_lens=self.mistake != "v_lens_not_updated")
        self.evicted = True

    def trim(self, policy, **kw):
        T = self._evictable_len()
        keep = keep_indices(policy, T, **kw)
        if keep is not None:
            self.keep_tokens(keep)
        elif self.mistake == "noop_trim_reallocates":
            self.k.alloc += 1
            self.v.alloc += 1

    def chunk_summarize(self, chunk_size, keep_last):
        T = self._evictable_len()
        if T - min(keep_last, T) <= 0:
            return
        self.k.chunk_pool(chunk_size, keep_last)
        self.v.chunk_pool(chunk_size, keep_last, move_lens=self.mistake != "v_lens_not_updated")
        self.evicted = True

    def evict_by_scores(self, scores, budget, prefix_len=0, recent=0, pool=1):
        T = self._evictable_len()
        if scores.shape[-1] != T:
            raise ValueError(f"kvq: evict_by_scores takes scores of shape [..., T = {T}]")
        keep = key_score_cases.np_keep_top_scores(self.reduce_scores(scores), budget, prefix_len, recent, pool)
        if keep is not None:
            self.keep_tokens(keep)
        return keep

    def compress_prompt(self, obs_queries, budget, prefix_len=0, pool=1):
        T = self._evictable_len()
        table = np.zeros((obs_queries[0].shape[0], self.k.H, T), np.float32)
        for layer, q in enumerate(obs_queries):
            table = (table + self.key_scores(layer, q).astype(np.float32)).astype(np.float32)
        return self.evict_by_scores(table, budget, prefix_len, recent=obs_queries[0].shape[2], pool=pool)


# ------------------------------------------------------------------------------------------------------------ the driver

def ratio(got, ref, dtype):
    """worst |got - ref| / the suite's standard tolerance (tests.gpu_harness.within_standard); inf when not finite"""
    got = np.asarray(got, np.float64)
    if got.shape != ref.shape or not np.isfinite(got).all():
        return float("inf")
    lim = TOL[dtype] * (np.abs(ref) + np.abs(ref).max())
    return float((np.abs(got - ref) / np.maximum(lim, 1e-30)).max())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


EVICTIONS = ("keep_tokens", "trim", "chunk_summarize", "score_evict", "compress_prompt")


def run_script(subject, script, mode, dtype, name="script", report=None):
    """Apply ``script`` to ``subject`` and to a fresh :class:`ShadowCache`; raise :class:`StepFailure` at the first step
    whose results or state differ (see the module docstring). ``report``: a dict that receives the worst output ratio per op."""
    assert not os.environ.get("KVQ_STORE_CAP_EXACT"), \
        "the life-cycle scripts predict capacities of the form 16 n + 8: unset KVQ_STORE_CAP_EXACT (a measurement knob)"
    sh = ShadowCache(L, mode, dtype)
    prev = None
    for i, (op, kw) in enumerate(script):
        def fail(check, detail, r=None):
            raise StepFailure(name, i, op, check, detail, r)

        def output(got, ref, what):
            r = ratio(got, ref, dtype)
            if report is not None:
                report[op] = max(report.get(op, 0.0), r)
            if r > 1.0:
                fail("output", f"{what}: worst error {r:.2f}x the tolerance", r)

        def masses(layer, q):
            got = subject.key_scores(layer, q)
            ref = sh.key_scores(layer, q)
            output(got, ref, f"key_scores layer {layer}")
            rows = (HQ // HKV) * (1 if q.ndim == 3 else q.shape[2])
            if not np.allclose(np.asarray(got, np.float64).sum(-1), rows, rtol=1e-4, atol=0):
                fail("output", f"key_scores layer {layer}: masses sum to {np.asarray(got).sum(-1).tolist()}, not {rows}", float("inf"))
            return np.asarray(got, np.float32)

        subject.launches()  # clears the kernel log
        kw = dict(kw)
        noop = kw.pop("noop", False)
        if op in ("init_from_prompt_past", "append_from_past", "reserve", "keep_tokens", "chunk_summarize"):
            getattr(subject, op)(**kw)
            getattr(sh, op)(**kw)
        elif op == "trim":
            subject.trim(kw["policy"], **kw["args"])
            sh.trim(kw["policy"], **kw["args"])
        elif op in ("attend", "extend"):
            ref = getattr(sh, op)(**kw)  # from the shadow's state BEFORE the call (an appending call moves it afterwards)
            output(getattr(subject, op)(**kw), ref, f"layer {kw['layer']}")
        elif op == "key_scores":
            masses(kw["layer"], kw["q"])
        elif op == "score_evict":
            m = masses(kw["layer"], kw["q"])
            args = dict(budget=kw["budget"], prefix_len=kw["prefix_len"], recent=kw["recent"], pool=kw["pool"])
            want = key_score_cases.np_keep_top_scores(subject.reduce_scores(m), **args)
            kept = subject.evict_by_scores(m, **args)
            if want is None or kept != want:
                fail("kept", f"kept {kept}, the top-score rule on the subject's own masses gives {want}")
            sh.keep_tokens(want)
        elif op == "compress_prompt":
            obs = kw["obs_queries"]
            table = None
            for layer, q in enumerate(obs):
                m = masses(layer, q)
                table = m if table is None else (table + m).astype(np.float32)  # what the accumulating calls hold
            args = dict(budget=kw["budget"], prefix_len=kw["prefix_len"], pool=kw["pool"])
            want = key_score_cases.np_keep_top_scores(subject.reduce_scores(table), recent=obs[0].shape[2], **args)
            kept = subject.compress_prompt(obs, **args)
            if want is None or kept != want:
                fail("kept", f"kept {kept}, the top-score rule on the subject's own masses gives {want}")
            sh.keep_tokens(want)
        elif op == "staging":
            want = sh.dequantised()
            sh.to_past_key_values()
            inc = subject.to_past_key_values()
            full = subject.to_past_key_values(copy=True)
            for what, got in (("copy=True", full), ("the incremental view", inc)):
                if len(got) != L or not all(_same(a, b) for x, y in zip(got, want) for a, b in zip(x, y)):
                    fail("staging", f"to_past_key_values: {what} is not the dequantised state")
        elif op == "raises":
            for who, c in (("subject", subject), ("shadow", sh)):
                try:
                    if kw["op"] == "score_evict":
                        T = max(sh.k.lens)
                        c.evict_by_scores(np.ones((B, HKV, T), np.float32), **kw["args"])
                    elif kw["op"] == "trim":
                        c.trim(kw["args"]["policy"], **kw["args"]["args"])
                    else:
                        getattr(c, kw["op"])(**kw["args"])
                except ValueError:
                    continue
                fail("raises", f"{kw['op']} on the {who} did not raise ValueError")
        elif op == "expect":
            st = sh.state()
            if (st["kcap"], st["vcap"]) != (kw["cap"],) * 2 or st["klens"] != [kw["T"]] * L:
                fail("cap", f"the script's own literal: capacity {kw['cap']} at T = {kw['T']}, the shadow has {st['kcap']} / {st['klens']}")
        else:
            raise AssertionError(f"unknown op {op!r}")
        # ---- the state, after every step
        got, want = subject.state(), sh.state()
        for which in ("k", "v"):
            lens, wlens = got[which + "lens"], want[which + "lens"]
            if lens != wlens:
                fail("lens", f"{which} store lens {lens}, expected {wlens}")
            cap, wcap = got[which + "cap"], want[which + "cap"]
            (q, s), (wq, ws) = got[which], want[which]
            dims = (q.shape[3], s.shape[1]) if q is not None else (0, 0)
            if cap != wcap or dims != (wcap, wcap):
                fail("cap", f"{which} store capacity {cap} (tensors {dims}), expected {wcap}")
            if prev is not None and cap < prev[which + "cap"]:
                fail("cap", f"{which} store capacity shrank from {prev[which + 'cap']} to {cap}")
            if op in EVICTIONS and prev is not None and max(lens) <= prev[which + "cap"] and cap != prev[which + "cap"]:
                fail("cap", f"{which} store: an eviction whose result fits changed the capacity {prev[which + 'cap']} -> {cap}")
            for g in range(L):
                T = lens[g]
                if not np.array_equal(q[g, :, :, :T], wq[g, :, :, :T]):
                    bad = sorted(set(np.nonzero((q[g, :, :, :T] != wq[g, :, :, :T]).any(axis=(0, 1, 3)))[0].tolist()))
                    fail("bits", f"{which} codes of layer {g} differ at tokens {bad[:8]} of {T}")
                if not np.array_equal(s[g, :T].view(np.uint32), ws[g, :T].view(np.uint32)):
                    bad = np.nonzero(s[g, :T].view(np.uint32) != ws[g, :T].view(np.uint32))[0].tolist()
                    fail("bits", f"{which} scale words of layer {g} differ at tokens {bad[:8]} of {T}")
        if got["layer_lens"] != want["layer_lens"]:
            fail("lens", f"len(layers[i]) {got['layer_lens']}, expected {want['layer_lens']}")
        Bs, Hs, Ds = sh.k.B, sh.k.H, sh.k.D
        wbytes = sum(O.estimated_bytes(mode, 1, Bs, Hs, T, Ds, 2) for T in want["klens"])
        if got["bytes"] != wbytes:
            fail("lens", f"estimated_bytes() {got['bytes']}, expected {wbytes}")
        if noop:
            if prev is not None and got["alloc"] != prev["alloc"]:
                fail("alloc", "a call that changes nothing reallocated the stores")
            log = subject.launches()
            if log:
                fail("launches", f"a call that changes nothing launched {log}")
        if op == "raises" and prev is not None and got["alloc"] != prev["alloc"]:
            fail("alloc", "a refused call reallocated the stores")
        if op == "attend" and kw.get("append"):
            log = subject.launches()
            if getattr(subject, "native", False) and (not log or not all(n.startswith("decode_attn") for n in log)):
                fail("launches", f"an appending decode step is kvq_decode_step's launches, not a quantise launch of its own: {log}")
        prev = dict(got, k=None, v=None)


# ------------------------------------------------------------------------------------------------------------- scripts

class _Builder:
    """Writes a script while running a correct shadow, so that every query can aim at what the store holds."""

    def __init__(self, mode, dtype, D, seed):
        self.mode, self.dtype, self.D = mode, dtype, D
        self.rng = np.random.default_rng([seed, D, len(mode), len(dtype)])
        self.sh = ShadowCache(L, mode, dtype)
        self.H = hadamard(D)
        self.sm = D ** -0.5
        self.serial = 0
        self.steps = []
        self.ghost = None  # [L][B,Hkv,D]: a key that was evicted; the next attention call aims at it as well

    @property
    def T(self):
        return self.sh.k.lens[0]

    def add(self, _op, **kw):
        self.steps.append((_op, kw))

    def expect(self, cap, T):
        self.add("expect", cap=cap, T=T)

    # -- inputs -------------------------------------------------------------------------------------------------------
    def tokens(self, n):
        """[L] x (k, v) [B,Hkv,n,D] in the compute dtype: token j carries +-amp x one Hadamard direction per kv head"""
        out = []
        base = self.serial
        self.serial += n
        for _ in range(L):
            k = self.rng.standard_normal((B, HKV, n, self.D)) * 0.1
            v = self.rng.standard_normal((B, HKV, n, self.D))
            for j in range(n):
                t = base + j
                for b in range(B):
                    for g in range(HKV):
                        i = t + 7 * g + 3 * b
                        sign = 1.0 if (i // (self.D - 2)) % 2 == 0 else -1.0
                        k[b, g, j] += sign * (1.0 + 0.5 * (t % 2)) * self.H[2 + i % (self.D - 2)]
            out.append((narrow(k, self.dtype), narrow(v, self.dtype)))
        return out

    def aim(self, targets):
        """float64 [B,Hq,D]: a query that scores AIM nats on each key of ``targets`` ([B,Hkv,D] float64 each)"""
        nq = HQ // HKV
        q = self.rng.standard_normal((B, HQ, self.D)) * 0.02
        for kd in targets:
            n2 = (kd * kd).sum(axis=-1, keepdims=True)
            q += np.repeat(AIM * kd / (self.sm * np.maximum(n2, 1e-12)), nq, axis=1)
        return q

    def _stored_targets(self, layer, extra=()):
        t = [self.sh.key_at(layer, self.sh.k.lens[layer] - 1)] + [self.sh.key_at(layer, s) for s in extra]
        if self.ghost is not None:
            t.append(self.ghost[layer])
        return t

    def mods(self, variant, layer, q, kn, ext):
        """the keyword arguments of a variant, a tuple of names out of :data:`VARIANTS`: a window that cuts, key starts with
        one row that sees no stored key, attn_mod_cases' soft cap, its four kinds of sinks"""
        assert set(variant) <= set(VARIANTS), variant
        T = self.sh.k.lens[layer]
        kw = {}
        if "window" in variant:
            kw["window"] = WINDOW
        if "kv_start" in variant:
            kw["kv_start"] = np.array([0, T], np.int32)  # row 1 sees no stored key
        if "softcap" in variant:
            kw["softcap"] = attn_mod_cases.CAP
        if "sinks" in variant:
            k, v = self.sh.k, self.sh.v
            S = q.shape[2] if ext else 1
            c = types.SimpleNamespace(
                mode="extend" if ext else "decode", dtype=self.dtype, kinds=(k.kind, v.kind), D=self.D, sm=self.sm, B=B, Hq=HQ,
                Hkv=HKV, T=T, S=S, q=q if ext else q[:, :, None], kn=kn, vn=kn, window=kw.get("window", 0),
                kv_start=None if "kv_start" not in kw else [int(x) for x in kw["kv_start"]],
                kq=k.q[layer][:, :, :T], ks=k.s[layer][:T], vq=v.q[layer][:, :, :T], vs=v.s[layer][:T])
            kw["sinks"] = attn_mod_cases.make_sinks(c, kw.get("softcap", 0.0))
        return kw

    # -- steps --------------------------------------------------------------------------------------------------------
    def prompt(self, n=PROMPT):
        past = self.tokens(n)
        self.add("init_from_prompt_past", past=past)
        self.sh.init_from_prompt_past(past)
        assert n == PROMPT
        self.expect(CAPS[0], n)

    def decode(self, append=True, layers=range(L), with_new=True, variant=()):
        """one decode step: per layer a query aimed at the last stored token, the new token (and the ghost); under a window
        also at the window's first key and at the key below it, which must stay unseen. Tokens that are not appended do not
        use up serial numbers (their directions are free again)."""
        serial = self.serial
        new = self.tokens(1)
        if not append:
            self.serial = serial
        for layer in layers:
            kn, vn = (new[layer][0][:, :, 0], new[layer][1][:, :, 0]) if with_new else (None, None)
            T = self.sh.k.lens[layer]
            extra = ()
            if "window" in variant:
                p = T if with_new else T - 1
                extra = (p - WINDOW + 1, p - WINDOW)
            targets = self._stored_targets(layer, extra) + ([widen(kn, self.dtype)] if with_new else [])
            q = narrow(self.aim(targets), self.dtype)
            kw = dict(layer=layer, q=q, k_new=kn, v_new=vn, append=append)
            if variant:
                kw.update(self.mods(variant, layer, q, kn, False))
            self.add("attend", **kw)
            self.sh.attend(**kw)
        if append and list(layers) == list(range(L)):
            self.ghost = None

    def chunk(self, S, append=True, variant=()):
        serial = self.serial
        new = self.tokens(S)
        if not append:
            self.serial = serial
        for layer in range(L):
            kn, vn = new[layer]
            kn64 = widen(kn, self.dtype)
            q = np.empty((B, HQ, S, self.D))
            for s in range(S):
                targets = [kn64[:, :, s]] + ([kn64[:, :, s + 1]] if s + 1 < S else [])
                if s == 0 and self.sh.k.lens[layer]:
                    targets += self._stored_targets(layer)
                q[:, :, s] = self.aim(targets)
            q = narrow(q, self.dtype)
            kw = dict(layer=layer, q=q, k_new=kn, v_new=vn, append=append)
            if variant:
                kw.update(self.mods(variant, layer, q, kn, True))
            self.add("extend", **kw)
            self.sh.extend(**kw)
        if append:
            self.ghost = None

    def scores_query(self, layer, S):
        """[B,Hq,S,D] (S = 0: the 3-D decode form): row s aims at its own token, the stored token T - S + s"""
        T = self.T
        rows = [self.aim([self.sh.key_at(layer, T - max(S, 1) + s)]) for s in range(max(S, 1))]
        q = np.stack(rows, axis=2)
        return narrow(q[:, :, 0] if S == 0 else q, self.dtype)

    def _set_ghost(self, slot):
        self.ghost = [self.sh.key_at(layer, slot) for layer in range(L)]

    def evict(self, op, ghost=None, **kw):
        """an eviction step; ``ghost``: a slot of the store as it stands that the eviction is known to drop"""
        if ghost is not None:
            self._set_ghost(ghost)
        self.add(op, **kw)
        if op == "trim":
            self.sh.trim(kw["policy"], **kw["args"])
        else:
            getattr(self.sh, op)(**kw)

    def score_evict(self, S, **args):
        """key_scores of layer 0, then evict_by_scores on them (the run takes the subject's own masses); the ghost is a
        token the rule drops"""
        q = self.scores_query(0, S)
        m = self.sh.key_scores(0, q)
        keep = key_score_cases.np_keep_top_scores(self.sh.reduce_scores(m), **args)
        gone = sorted(set(range(self.T)) - set(keep))
        self._set_ghost(gone[len(gone) // 2])
        self.add("score_evict", layer=0, q=q, **args)
        self.sh.keep_tokens(keep)

    def to_65(self):
        """prompt 17 (capacity 24), a chunk of 8 (T 25, capacity 56), the incremental view at T 25, a chunk of 40 (T 65,
        capacity 120): staged then trails T by 40 tokens"""
        self.prompt()
        self.chunk(8)
        self.expect(CAPS[1], 25)
        self.add("staging")
        self.chunk(40)
        self.expect(CAPS[2], 65)


def build_script(name, mode, dtype, D, seed=0):
    """The script ``name`` (one of :data:`SCRIPTS`) for one configuration, as a list of ``(op, kwargs)``."""
    b = _Builder(mode, dtype, D, seed)
    if name == "growth":
        b.prompt()
        assert b.sh.k.cap == CAPS[0] == 24
        b.add("staging")  # staged = 17
        while b.T < CAPS[0]:
            b.decode()
        b.expect(CAPS[0], 24)  # exactly full
        b.decode(append=False)  # a full store plus a new token
        b.decode()  # grows to 56 inside the call, with a plan cached for the old store
        b.expect(CAPS[1], 25)
        b.add("staging")  # staged 17 -> 25 across the growth
        b.chunk(9)
        b.expect(CAPS[1], 34)
        b.chunk(31)  # 34 -> 65: grows to 120 inside extend, across the 64-token tile edge
        b.expect(CAPS[2], 65)
        past = b.tokens(1)
        b.add("append_from_past", past=past)
        b.sh.append_from_past(past)
        for layer in range(L):
            b.add("key_scores", layer=layer, q=b.scores_query(layer, 5))
            b.add("key_scores", layer=layer, q=b.scores_query(layer, 0))
        b.add("reserve", n=300)
        b.sh.reserve(300)
        b.expect(312, 66)
        b.decode()
        for layer in range(L):
            b.add("key_scores", layer=layer, q=b.scores_query(layer, 5))  # the workspace was sized for capacity 120
        b.add("staging")  # staged 25 -> 67 across two growths
    elif name == "evict":
        b.to_65()
        b.score_evict(5, budget=40, prefix_len=2, recent=5, pool=3)
        b.expect(CAPS[2], 40)
        b.decode()  # a new plan; slot 40; capacity still 120
        b.expect(CAPS[2], 41)
        b.add("staging")  # staged was 25 before the eviction
        b.evict("chunk_summarize", ghost=3, chunk_size=8, keep_last=6)
        b.expect(CAPS[2], 11)
        b.chunk(7)
        b.evict("trim", ghost=2, policy="strided", args=dict(window_size=4, stride=3, prefix_len=1))
        b.expect(CAPS[2], 10)
        b.decode(append=False)
        b.ghost = None
        b.add("staging")
        b.evict("trim", policy="sliding_window", args=dict(window_size=64), noop=True)  # keeps everything
        b.evict("keep_tokens", idx=[(3 * i) % 10 for i in range(130)])  # does not fit: the capacity grows, stage is dropped
        b.expect(136, 130)
        b.decode()
        b.add("staging")
        obs = [b.scores_query(layer, 4) for layer in range(L)]
        b.add("compress_prompt", obs_queries=obs, budget=30, prefix_len=2, pool=3)
        b.sh.compress_prompt(obs, budget=30, prefix_len=2, pool=3)
        b.expect(136, 30)
        b.decode()
        b.add("staging")
    elif name == "variants":
        b.to_65()
        b.evict("trim", ghost=0, policy="sliding_window", args=dict(window_size=60))
        b.chunk(3)
        for T in (63, 64, 65):
            assert b.T == T
            for variant in [(v,) for v in VARIANTS] + [VARIANTS]:
                b.decode(append=False, variant=variant)
                b.chunk(5, append=False, variant=variant)
            b.decode(append=False, with_new=False, variant=("kv_start",))  # row 1 sees no key at all: zeros
            b.decode(append=False, with_new=False, variant=("window",))
            if T == 63:
                b.decode()  # a plain appending step
            elif T == 64:  # an appending step under a window and sinks: the stored slot is the plain call's (the shadow's)
                b.decode(variant=("window", "sinks"))
        b.expect(CAPS[2], 65)
    elif name == "mid_walk":
        b.prompt()
        b.add("staging")
        b.decode(layers=[0])  # layer 0 holds 18 tokens, layer 1 still 17: a decode step half way through its layer walk
        b.add("raises", op="to_past_key_values", args={})
        b.add("raises", op="trim", args=dict(policy="sliding_window", args=dict(window_size=4)))
        b.add("raises", op="chunk_summarize", args=dict(chunk_size=4, keep_last=2))
        b.add("raises", op="score_evict", args=dict(budget=8, prefix_len=1, recent=2, pool=1))
        b.decode(layers=[1])  # finishing the walk then works
        b.expect(CAPS[0], 18)
        b.add("staging")
        b.evict("trim", ghost=0, policy="sliding_window", args=dict(window_size=4))
        b.decode()
        b.add("staging")
    else:
        raise ValueError(name)
    return b.steps


_SCRIPTS = {}


def script(name, mode, dtype, D):
    """:func:`build_script`, built once per (script, configuration) and shared by the tests (read-only)"""
    key = (name, mode, dtype, D)
    if key not in _SCRIPTS:
        _SCRIPTS[key] = build_script(name, mode, dtype, D)
    return _SCRIPTS[key]
