"""Decode with attention computed straight from the quantised store (scope row N1, second form).

The reference dequantises the whole cache to fp16 before every forward
(``QuantizedKVCache.to_past_key_values``, reference src/quantization/ops.py:345-355, called from
src/benchmarking/benchmarker.py:470-471) and the model's attention then reads that fp16 copy. Here
the model's attention function IS the HIP kernel ``kvq_decode_attn``: it reads the INT8 / packed
INT4 rows and their per-token scales, adds the new token's exact K/V as one more softmax term
(what the reference's ``cat`` does), and no fp16 copy of the cache exists at any time — the
resident KV really is ``estimated_bytes()``.

Plumbing (transformers >= 4.54 / 5.x):

  * :class:`FusedQuantizedCache` owns a :class:`QuantizedKVCache` and hands the model a
    ``DynamicCache`` whose layers quantise the prompt's K/V into the store (2 launches per layer) and
    pass the new tokens' exact K/V on to the attention function; a decode token is quantised by the
    same host call that attends (``kvq_decode_step``: one ctypes call and, for grouped-query shapes,
    one launch per layer and step);
  * ``kvq_fused`` is registered with transformers' ``AttentionInterface``; inside
    :func:`fused_attention` the model's ``_attn_implementation`` points at it. A single-token
    query runs ``kernels.decode_attn`` on the layer's store; a prompt (empty cache) runs exact
    causal SDPA over the prompt's own K/V, as the reference's un-quantised prompt forward does; a
    forward of several tokens into a non-empty cache (the next turn of a chat, a chunk of a long
    prompt, a speculative-decoding verify) runs ``kernels.extend_attn``: the stored tokens from the
    store, the chunk's exact K/V causally (the chunk itself is quantised into the store by the
    cache layer's ``update``, as a prompt is).
  * a mask function is registered under the same name: for a multi-token forward over a past and no
    padding it returns ``None`` (the kernel applies causality itself) where transformers would
    materialise a ``[B, 1, n, past + n]`` mask; anything else is left to ``sdpa_mask``.

Numerics: fp32 accumulation over exact integer x fp16 products; the rounding of each dequantised
value to fp16 that the reference's tuple path performs is skipped, so logits agree within fp16
tolerance, not bit-for-bit (tests/test_gpu_attn.py, tests/test_gpu_benchmarker.py).
Sliding-window layers (Mistral, Qwen2 / 3 with ``use_sliding_window``, Gemma 3's local layers): the window of
each layer is resolved per call (the ``sliding_window`` keyword first, then ``module.sliding_window``; None = full
attention) and handed to the kernels, which read only the stored rows inside it; the store keeps every token, as the
reference's does. A prompt longer than the window runs SDPA with an explicit band mask.

Limits (fail loudly): fp16 / bf16 models, head_dim in {32, 64, 128, 256}, at most 8 query heads
per kv head (16 at head_dim 64 / 128), no padding mask unless the cache was told of a LEFT-padded batch
(``FusedQuantizedCache.set_left_padding``: per-row key starts go to the ``kvq_*_padded`` kernels), a multi-token
forward into a non-empty cache only at head_dim 64 / 128 and not in graph mode (``t_dev``). Soft-capped layers (Gemma 2's
``attn_logit_softcapping``) and attention sinks (gpt-oss's ``s_aux``) are refused (``_reject_unsupported_variants``) unless
the cache was built with ``FusedQuantizedCache(..., score_modifiers=True)``: then the cap (the ``softcap`` keyword, else
``module.attn_logit_softcapping``) and the sinks (the ``s_aux`` / ``sinks`` keyword, else ``module.sinks``; converted to fp32
``[Hq]`` once per module) go to the ``kvq_*_ex`` kernels, and the prompt forward runs explicit eager attention (scores, cap,
mask, softmax with the sink column), since SDPA has neither modifier.
"""
from __future__ import annotations

import contextlib
import weakref
from typing import Optional

import torch

from .. import kernels
from .ops import QuantizedKVCache

try:
    from transformers import AttentionInterface
    from transformers.cache_utils import DynamicCache, DynamicLayer
    from transformers.masking_utils import AttentionMaskInterface, prepare_padding_mask, sdpa_mask
except Exception:  # pragma: no cover - older transformers: the staged / tuple paths are used instead
    AttentionInterface = None
    DynamicCache = DynamicLayer = None

ATTN_NAME = "kvq_fused"
_ACTIVE: Optional["FusedQuantizedCache"] = None


def available() -> bool:
    return AttentionInterface is not None and DynamicLayer is not None


if DynamicLayer is not None:

    class _FusedLayer(DynamicLayer):
        """One layer of the HF cache, backed by group ``index`` of the K and V stores."""

        def __init__(self, owner: "FusedQuantizedCache", index: int):
            super().__init__()
            self._owner = owner
            self._index = index
            self.is_initialized = True
            self.past = 0  # tokens in the store before the forward in flight
            self.pending = False  # the new token still has to be quantised (done by the attention call)
            self.plan = None  # kernels.DecodeStepPlan of this layer
            self.keys = self.values = None  # nothing dequantised is ever kept

        def update(self, key_states: torch.Tensor, value_states: torch.Tensor, *args, **kwargs):
            qc, i = self._owner.qcache, self._index
            self.past = qc._k.lens[i]
            self.dtype, self.device = key_states.dtype, key_states.device
            if key_states.shape[-2] == 1 and self.past > 0:
                # decode: the attention function quantises this token into slot `past` in the same
                # host call that attends (kvq_decode_step); only the capacity is settled here
                if self._owner.t_dev is None:  # graph mode: capacity was reserved up front, nothing may reallocate
                    qc._k.reserve(self.past + 1)
                    qc._v.reserve(self.past + 1)
                self.pending = True
                return key_states, value_states
            if key_states.shape[-2] > 1 and self.past > 0 and self._owner.t_dev is not None:
                raise RuntimeError("kvq: a multi-token forward into the quantised cache is not supported in graph mode")
            # prompt, or a chunk behind a non-empty store (its attention reads the store only up to `past`): a dense
            # copy takes the single-pass quantise path; one launch per store
            qc._k.append([key_states.contiguous()], g0=i)
            qc._v.append([value_states.contiguous()], g0=i)
            self.pending = False
            return key_states, value_states  # the new tokens' exact K/V go on to the attention function

        def get_seq_length(self) -> int:
            return self._owner.qcache._k.lens[self._index]


class FusedQuantizedCache:
    """A :class:`QuantizedKVCache` the model appends to and attends over directly."""

    def __init__(self, n_layers: int, mode: str = "int8", device: str = "cuda",
                 compute_dtype: torch.dtype = torch.float16, reserve: int = 0, score_modifiers: bool = False):
        if not available():
            raise RuntimeError("kvq: this transformers version has no AttentionInterface / DynamicLayer")
        self.qcache = QuantizedKVCache(n_layers=n_layers, mode=mode, device=device, compute_dtype=compute_dtype)
        self.qcache._fused_owner = weakref.ref(self)  # eviction inside the store is refused while t_dev is set
        if reserve:
            self.qcache.reserve(reserve)
        self.cache = DynamicCache()
        self.cache.layers = [_FusedLayer(self, i) for i in range(n_layers)]
        self._ws: Optional[torch.Tensor] = None
        self._ws_key = None
        self._ws_T = 0
        self._ext_ws: Optional[torch.Tensor] = None
        # transformers materialises the (all-true) causal mask of a single-token query while a stream is being
        # captured instead of skipping it; a driver that guarantees un-padded prompts (the graphed decode of
        # KVCacheBenchmarker) sets this so that the mask is ignored rather than refused
        self.ignore_decode_mask = False
        # graph mode (KVCacheBenchmarker.graph_decode): the stored-token count lives in this one-element int32
        # GPU tensor, every decode step runs kvq_decode_step_dev with step-independent launch arguments, and the
        # DRIVER advances the host-side lengths (once per replayed step) — see _fused_attention_forward
        self.t_dev: Optional[torch.Tensor] = None
        self.t_bound = 0
        # left-padded batches (set_left_padding): per-row first real key, int32 on the device, for the life of the cache
        self.kv_start: Optional[torch.Tensor] = None
        # opt-in to logit soft-capping and attention sinks (Gemma 2, gpt-oss): the fused forward then hands them to the
        # kvq_*_ex kernels instead of refusing the layer; sinks are kept per module as fp32 [Hq] (one pointer per layer for
        # the life of the cache, so a captured decode step replays with it)
        self.score_modifiers = bool(score_modifiers)
        self._sinks: dict = {}

    def set_left_padding(self, attention_mask: torch.Tensor) -> torch.Tensor:
        """Opt in to a LEFT-padded batch: ``attention_mask`` is the tokenizer's 2-D ``[B, prompt_len]`` mask (0 = padding),
        every row zeros then ones with at least one 1. Keeps ``kv_start[b]`` = row ``b``'s first real position (int32, on
        the cache's device) for the life of the cache: the prompt forward then takes the model's materialised mask into
        SDPA, and decode / multi-token forwards over the store pass ``kv_start`` to the padded kernels
        (``kvq_*_padded``) instead of refusing the mask. Right padding, holes and all-padding rows are refused: the
        store has ONE scale per token slot for all rows, so only per-row starts can share it. Returns ``kv_start``."""
        m = torch.as_tensor(attention_mask)
        if m.dim() != 2 or m.size(0) < 1 or m.size(1) < 1:
            raise RuntimeError(f"kvq: set_left_padding takes the 2-D [B, prompt_len] attention mask, got shape {tuple(m.shape)}")
        real = (m != 0).cpu()
        if not bool(real.any(dim=1).all()):
            raise RuntimeError("kvq: set_left_padding: a row of the attention mask is all padding")
        start = real.int().argmax(dim=1)  # first 1 of each row
        cols = torch.arange(real.size(1))[None, :]
        if not bool((real == (cols >= start[:, None])).all()):
            raise RuntimeError("kvq: set_left_padding takes LEFT padding only (every row zeros, then ones): "
                               "right-padded rows or holes cannot share the store's per-slot scales")
        self.kv_start = start.to(torch.int32).to(self.qcache._k.device).contiguous()
        return self.kv_start

    def workspace(self, B: int, Hq: int, Hkv: int, T: int, D: int, device) -> torch.Tensor:
        """Scratch for the split partials, sized once for the reserved capacity (decode never reallocates
        and asks the library for the size only when the shape or the capacity changes)."""
        key = (B, Hq, Hkv, D, self.qcache._k.cap)
        if self._ws is None or self._ws_key != key or T > self._ws_T:
            cap = max(self.qcache._k.cap, T, 1)
            # the per-T size is not monotone in T: ask for the maximum over every T <= cap
            self._ws = torch.empty(kernels.decode_attn_workspace_cap(B, Hq, Hkv, cap, D), dtype=torch.float32, device=device)
            self._ws_key, self._ws_T = key, cap
        return self._ws

    def extend_workspace(self, B: int, Hq: int, Hkv: int, T: int, S: int, D: int, device) -> torch.Tensor:
        """Scratch of a multi-token forward (kernels.extend_attn), sized at the reserved capacity (the size is
        non-decreasing in the stored-token count) and grown when a larger chunk needs more."""
        need = max(kernels.extend_attn_workspace(B, Hq, Hkv, max(self.qcache._k.cap, T), S, D), 1)
        if self._ext_ws is None or self._ext_ws.numel() < need or self._ext_ws.device != torch.device(device):
            self._ext_ws = torch.empty(need, dtype=torch.float32, device=device)
        return self._ext_ws

    def estimated_bytes(self) -> int:
        return self.qcache.estimated_bytes()


# what transformers passes for attention variants this kernel does not implement: plain softmax over
# EVERY stored token is all it computes, so any of these must stop the run instead of being ignored
_UNSUPPORTED_KWARGS = ("sliding_window", "softcap", "s_aux", "sinks")
_UNSUPPORTED_MODULE_ATTRS = ("sliding_window", "sinks", "attn_logit_softcapping")


def _reject_unsupported_variants(module, kwargs, implemented=()) -> None:
    """Sliding-window (Mistral / Qwen2 / Gemma), logit soft-capping (Gemma 2) and attention sinks reach an
    attention-interface function as keyword arguments or module attributes. Raise on any of them but the names in
    ``implemented`` (the fused forward passes ``("sliding_window",)``: its kernels apply the window)."""
    for name in _UNSUPPORTED_KWARGS:
        if name in implemented:
            continue
        if kwargs.get(name) is not None:
            raise RuntimeError(f"kvq: fused attention over the quantised store does not implement '{name}' "
                               f"(got {kwargs[name]!r}); use the staged path (fused_attention=False) for this model")
    for name in _UNSUPPORTED_MODULE_ATTRS:
        if name in implemented:
            continue
        if getattr(module, name, None) is not None:
            raise RuntimeError(f"kvq: fused attention over the quantised store does not implement the attention "
                               f"variant this layer is configured with ({type(module).__name__}.{name} = "
                               f"{getattr(module, name)!r}); use the staged path (fused_attention=False)")


_MODIFIER_NAMES = ("softcap", "s_aux", "sinks", "attn_logit_softcapping")


def _layer_softcap(module, kwargs) -> float:
    """The layer's logit soft cap for this call: the ``softcap`` keyword wins, else ``module.attn_logit_softcapping``;
    None = none (0.0)."""
    c = kwargs.get("softcap")
    if c is None:
        c = getattr(module, "attn_logit_softcapping", None)
    if c is None:
        return 0.0
    c = float(c)
    if not (0.0 < c < float("inf")):
        raise RuntimeError(f"kvq: logit soft cap must be a finite positive number, got {c!r}")
    return c


def _layer_sinks(owner, module, kwargs, Hq: int, device) -> Optional[torch.Tensor]:
    """The layer's attention sinks for this call as a contiguous fp32 ``[Hq]`` tensor on ``device``: the ``s_aux`` keyword,
    else ``sinks``, else ``module.sinks``; None = none. Converted once per (module, source tensor) and kept on the
    cache, so every later step (and a captured graph) sees the same pointer."""
    src = kwargs.get("s_aux")
    if src is None:
        src = kwargs.get("sinks")
    if src is None:
        src = getattr(module, "sinks", None)
    if src is None:
        return None
    if not isinstance(src, torch.Tensor) or src.numel() != Hq:
        raise RuntimeError(f"kvq: attention sinks must be a tensor of one logit per query head ({Hq}), got "
                           f"{tuple(src.shape) if isinstance(src, torch.Tensor) else type(src).__name__}")
    key = id(module)
    hit = owner._sinks.get(key)
    if hit is None or hit[0] is not src or hit[1] != src._version or hit[2].device != torch.device(device):
        hit = owner._sinks[key] = (src, src._version, src.detach().reshape(Hq).to(device=device, dtype=torch.float32).contiguous())
    return hit[2]


def _eager_prompt_attention(query, key, value, mask, scale: float, softcap: float, sinks) -> torch.Tensor:
    """The prompt forward with a score modifier, as transformers' ``eager_attention_forward`` of Gemma 2 / gpt-oss computes
    it (SDPA has neither): scores, cap, mask, softmax over the keys and the head's sink column, the sink's probability
    dropped. ``mask``: bool ``[.., n, n]`` (True = visible) or additive. Returns ``[B, Hq, n, D]`` in the query's dtype.
    The reference's un-quantised prompt pass, not the hot path."""
    B, Hq, n, D = query.shape
    rep = Hq // key.shape[1]
    k = key.repeat_interleave(rep, dim=1) if rep > 1 else key
    v = value.repeat_interleave(rep, dim=1) if rep > 1 else value
    s = torch.matmul(query.float(), k.float().transpose(-1, -2)) * scale
    if softcap:
        s = torch.tanh(s / softcap) * softcap
    if mask.dtype == torch.bool:
        s = s.masked_fill(~mask, float("-inf"))
    else:
        s = s + mask.float()
    if sinks is not None:
        s = torch.cat([s, sinks.float().view(1, Hq, 1, 1).expand(B, Hq, n, 1)], dim=-1)
    p = torch.softmax(s - s.amax(dim=-1, keepdim=True), dim=-1)
    if sinks is not None:
        p = p[..., :-1]
    return torch.matmul(p, v.float()).to(query.dtype)


def _layer_window(module, kwargs) -> int:
    """The layer's sliding window for this call: the ``sliding_window`` keyword, else ``module.sliding_window``
    (Qwen2 mixes full and sliding layers, so per layer and per call); None = full attention (0)."""
    w = kwargs.get("sliding_window")
    if w is None:
        w = getattr(module, "sliding_window", None)
    if w is None:
        return 0
    if isinstance(w, bool) or int(w) != w or int(w) <= 0:
        raise RuntimeError(f"kvq: sliding_window must be a positive integer, got {w!r}")
    return int(w)


def _fused_attention_forward(module, query, key, value, attention_mask=None, dropout: float = 0.0,
                             scaling: Optional[float] = None, **kwargs):
    """transformers attention-interface function: ``(attn_output [B, n, Hq, D], None)``."""
    owner = _ACTIVE
    if owner is None:
        raise RuntimeError("kvq: the 'kvq_fused' attention runs only inside fused_attention(model, cache)")
    if dropout:
        raise RuntimeError("kvq: fused decode attention is inference-only (dropout must be 0)")
    # the sliding window is implemented by the kernels of a FusedQuantizedCache; a cache built with score_modifiers=True
    # also takes the soft cap and the sinks; everything else stays refused
    mods = bool(getattr(owner, "score_modifiers", False))
    implemented = ("sliding_window",) if isinstance(owner, FusedQuantizedCache) else ()
    _reject_unsupported_variants(module, kwargs, implemented=implemented + (_MODIFIER_NAMES if mods else ()))
    window = _layer_window(module, kwargs)
    B, Hq, n, D = query.shape
    softcap = _layer_softcap(module, kwargs) if mods else 0.0
    sinks = _layer_sinks(owner, module, kwargs, Hq, query.device) if mods else None
    Hkv = key.shape[1]
    scale = float(scaling) if scaling is not None else D ** -0.5
    layer = owner.cache.layers[module.layer_idx]
    if n > 1 and layer.past > 0:
        # several tokens behind a non-empty store: the stored tokens [0, past) from the store, the chunk's exact
        # K/V causally (update() has already quantised the chunk into slots past .. past + n - 1)
        if owner.t_dev is not None:
            raise RuntimeError("kvq: a multi-token forward into the quantised cache is not supported in graph mode")
        kv_start = getattr(owner, "kv_start", None)
        if attention_mask is not None and kv_start is None:
            raise RuntimeError("kvq: fused multi-token attention does not take a padding mask")
        qc, i = owner.qcache, module.layer_idx
        out = torch.empty(B, n, Hq, D, dtype=query.dtype, device=query.device)
        kernels.extend_attn(query, qc._k.q[i], qc._k.scales[i], qc._k.kind, qc._v.q[i], qc._v.scales[i], qc._v.kind,
                            layer.past, key, value, out.transpose(1, 2),
                            owner.extend_workspace(B, Hq, Hkv, layer.past, n, D, query.device), scale, window,
                            kv_start=kv_start,  # left padding: the materialised mask is ignored, the kernel applies the starts
                            softcap=softcap, sinks=sinks)
        layer.pending = False
        return out, None
    if n > 1 or layer.past == 0:
        # the prompt forward (or the very first token): exact attention over the tokens' own K/V,
        # like the reference's un-quantised prompt pass (benchmarker.py:445-449)
        if attention_mask is not None:
            if getattr(owner, "kv_start", None) is None:
                raise RuntimeError("kvq: fused attention does not take a padding mask")
            # a left-padded prompt: the model's materialised mask (causal, padding and the layer's window) goes to SDPA. A
            # query at a PAD position sees no key there; it is given its own key, so that its output, and with it the K / V
            # the next layer produces at that position, stays finite: they enter the abs-max of the slot's shared scale.
            m = attention_mask[..., :n, :n]
            eye = torch.eye(n, dtype=torch.bool, device=m.device)
            if m.dtype == torch.bool:
                m = m | (~m.any(dim=-1, keepdim=True) & eye)
            else:
                dead = (m == float("-inf")).all(dim=-1, keepdim=True) | (m <= torch.finfo(m.dtype).min).all(dim=-1, keepdim=True)
                m = m.masked_fill(dead & eye, 0.0)
            if softcap or sinks is not None:
                return _eager_prompt_attention(query, key, value, m, scale, softcap, sinks).transpose(1, 2).contiguous(), None
            out = torch.nn.functional.scaled_dot_product_attention(query, key, value, attn_mask=m, scale=scale,
                                                                   enable_gqa=Hkv != Hq)
            return out.transpose(1, 2).contiguous(), None
        if softcap or sinks is not None:  # a score modifier: explicit eager attention under the same causal / band mask
            i = torch.arange(n, device=query.device)
            vis = i[None, :] <= i[:, None]
            if window and n > window:
                vis = vis & (i[None, :] > i[:, None] - window)
            return _eager_prompt_attention(query, key, value, vis, scale, softcap, sinks).transpose(1, 2).contiguous(), None
        if window and n > window:  # causal AND inside the window: key j visible to query i iff i - window < j <= i
            i = torch.arange(n, device=query.device)
            band = (i[None, :] <= i[:, None]) & (i[None, :] > i[:, None] - window)
            out = torch.nn.functional.scaled_dot_product_attention(query, key, value, attn_mask=band, scale=scale,
                                                                   enable_gqa=Hkv != Hq)
        else:
            out = torch.nn.functional.scaled_dot_product_attention(query, key, value, is_causal=n > 1, scale=scale,
                                                                   enable_gqa=Hkv != Hq)
        return out.transpose(1, 2).contiguous(), None
    kv_start = getattr(owner, "kv_start", None)  # left padding: the materialised mask is ignored, the kernels apply the starts
    if attention_mask is not None and not owner.ignore_decode_mask and kv_start is None:
        raise RuntimeError("kvq: fused decode attention does not take a padding mask")
    qc, i = owner.qcache, module.layer_idx
    T = layer.past
    out = torch.empty(B, 1, Hq, D, dtype=query.dtype, device=query.device)
    q3 = query[:, :, 0]
    plan = layer.plan
    if plan is None or plan.key != (qc._k.q[i].data_ptr(), qc._v.q[i].data_ptr(), query.dtype, B, Hq, D):
        plan = layer.plan = kernels.DecodeStepPlan(q3, qc._k.q[i], qc._k.scales[i], qc._k.kind, qc._v.q[i],
                                                   qc._v.scales[i], qc._v.kind, qc._k.eps)
    if owner.t_dev is not None:
        # device-side T: the same launches serve every later step (captured once, replayed per token); the
        # host-side lengths are the driver's to advance
        kernels.decode_step_dev(plan, q3, key[:, :, 0], value[:, :, 0], owner.t_dev, owner.t_bound, out[:, 0],
                                owner.workspace(B, Hq, Hkv, owner.t_bound, D, query.device), scale, window, kv_start=kv_start,
                                softcap=softcap, sinks=sinks)
        layer.pending = False
        return out, None
    kernels.decode_step(plan, q3, key[:, :, 0], value[:, :, 0], T, out[:, 0],
                        owner.workspace(B, Hq, Hkv, T, D, query.device), scale, window, kv_start=kv_start,
                        softcap=softcap, sinks=sinks)
    qc._k.lens[i] = qc._v.lens[i] = T + 1  # the step appended the token
    layer.pending = False
    return out, None


def _fused_mask(batch_size: int, q_length: int, kv_length: int, *args, attention_mask=None, **kwargs):
    """Mask interface of ``kvq_fused``. A multi-token forward over a past (``kv_length > q_length > 1``) without
    padding gets ``None``: kvq_extend_attn applies the lower-right-aligned causal mask itself, and transformers would
    otherwise materialise it (``_ignore_causal_mask_sdpa`` skips only single-token and past-free queries). A real
    padding mask, a local window or a custom mask function goes to ``sdpa_mask`` and reaches the attention function,
    which refuses it (unless the active cache was told of a left-padded batch: see below). A local-window call (``local_size``) without padding gets ``None`` too, decode or multi-token:
    the kernels apply the window. Every other call is exactly ``sdpa_mask``."""
    # A cache told of a LEFT-padded batch (set_left_padding), any forward over a past: the padded kernels apply the per-row
    # starts (and the window) themselves and the attention function ignores the mask, so none is materialised and the
    # padding mask is not read here (reading it is a device-to-host copy, which a stream capture of the decode step forbids).
    if getattr(_ACTIVE, "kv_start", None) is not None and kv_length > q_length:
        return None
    if kwargs.get("local_size") is not None:
        kv_offset = kwargs.get("kv_offset", args[1] if len(args) > 1 else 0)
        padding_mask = prepare_padding_mask(attention_mask, kv_length, kv_offset)
        if padding_mask is None or bool(padding_mask.all()):
            return None
        return sdpa_mask(batch_size, q_length, kv_length, *args, attention_mask=attention_mask, **kwargs)
    if (q_length > 1 and kv_length > q_length and kwargs.get("allow_is_causal_skip", True)
            and kwargs.get("local_size") is None):
        kv_offset = kwargs.get("kv_offset", args[1] if len(args) > 1 else 0)
        padding_mask = prepare_padding_mask(attention_mask, kv_length, kv_offset)
        if padding_mask is None or bool(padding_mask.all()):
            return None
    return sdpa_mask(batch_size, q_length, kv_length, *args, attention_mask=attention_mask, **kwargs)


@contextlib.contextmanager
def fused_attention(model, cache: FusedQuantizedCache):
    """Route ``model``'s attention through the quantised store of ``cache`` for the duration."""
    global _ACTIVE
    if not available():
        raise RuntimeError("kvq: this transformers version has no AttentionInterface / DynamicLayer")
    AttentionInterface.register(ATTN_NAME, _fused_attention_forward)
    AttentionMaskInterface.register(ATTN_NAME, _fused_mask)
    before = model.config._attn_implementation
    prev_active = _ACTIVE
    model.set_attn_implementation(ATTN_NAME)
    _ACTIVE = cache
    try:
        yield cache.cache
    finally:
        _ACTIVE = prev_active
        model.set_attn_implementation(before)


__all__ = ["FusedQuantizedCache", "fused_attention", "available", "ATTN_NAME"]
