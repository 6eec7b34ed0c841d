"""KV-cache quantisation on MI355X: the reference's ``src/quantization/ops.py`` surface over HIP.

Same names, arguments, return orders and exceptions as the reference
(reference src/quantization/__init__.py:12-19): ``quantize_int8_per_tensor``,
``quantize_int4_per_tensor_packed``, ``dequantize_int8_per_tensor``,
``dequantize_int4_per_tensor_packed``, ``QuantizedLayerKV``, ``QuantizedKVCache``.

What changed underneath (MI355X-first, results identical):
  * the reference keeps six Python lists of per-token tensors per layer and issues 2*L*T
    dequantise launches + 2*L T-way ``torch.cat`` per decode step (ops.py:213-269, :345-355).
    Here a KV set is ONE persistent buffer ``[G, B, H, Tcap, Dq]`` (G = layers) plus an fp32 scale
    table ``[G, Tcap]``; prefill quantises all layers x all tokens in one launch per K/V set,
    a decode append is one launch per set, and ``to_past_key_values`` is one launch per set.
  * no host synchronisation: scales never leave the device (the reference calls
    ``float(scale)`` per slice, ops.py:87,117).
  * arithmetic lives in libkvq_hip.so only; CPU tensors raise (no fallback).
"""
from __future__ import annotations

import os
import weakref

from typing import List, Optional, Sequence, Tuple

import torch

from .. import _lib, kernels
from ..cache.implementations import KEEP_INDEX_FNS, keep_indices_top_scores
from ..kernels import QDTYPE, packed_dim

_OUT_DTYPES = (torch.float16, torch.bfloat16, torch.float32)


# ----------------------------------------------------------------------------- per-tensor API


def _as_rows(x: torch.Tensor) -> torch.Tensor:
    """View an arbitrary tensor as [1, B, H, 1, D] (one scale over everything) without copying
    when it is a [B,H,1,D] slice — the shape QuantizedLayerKV.append feeds (ops.py:178-179)."""
    if x.dim() == 4 and x.size(2) == 1:
        return x.unsqueeze(0)
    D = x.size(-1)
    return x.reshape(1, 1, -1, 1, D)


def _quantize_per_tensor(x: torch.Tensor, eps: float, kind: str):
    _lib.require_gpu(x, "x")
    if x.numel() == 0:
        raise _lib.KvqError("kvq: cannot quantise an empty tensor")  # reference: abs().max() raises too
    xx = x.reshape(1) if x.dim() == 0 else x
    x5 = _as_rows(xx)
    Dq = packed_dim(kind, x5.size(4))
    q = torch.empty(tuple(xx.shape[:-1]) + (Dq,), dtype=QDTYPE[kind], device=x.device)
    scales = torch.empty(1, 1, dtype=torch.float32, device=x.device)
    ws = torch.empty(1, dtype=torch.float32, device=x.device)
    kernels.quant_tokens(x5, q.view(1, x5.size(1), x5.size(2), 1, Dq), scales, ws, kind, eps)
    if x.dim() == 0 and kind == "int8":
        q = q.reshape(())
    # stored scale: already rounded to x.dtype by the kernel, so this cast is exact (ops.py:30,65)
    return q, scales.reshape(()).to(x.dtype)


def quantize_int8_per_tensor(x: torch.Tensor, eps: float = 1e-8) -> Tuple[torch.Tensor, torch.Tensor]:
    """Symmetric per-tensor INT8: ``q = clamp(round(x/scale), -127, 127)``, ``scale = max(max|x|/127, eps)``
    computed in fp32 and returned rounded to ``x.dtype`` (reference ops.py:10-30)."""
    return _quantize_per_tensor(x, eps, "int8")


def quantize_int4_per_tensor_packed(x: torch.Tensor, eps: float = 1e-8) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """Symmetric per-tensor INT4 in [-8, 7], two values per byte along the last dim (even index
    in the high nibble; an odd last dim is padded). Returns ``(packed, scale, orig_last_dim)``
    (reference ops.py:33-65)."""
    q, s = _quantize_per_tensor(x, eps, "int4")
    return q, s, int(x.size(-1))


def _scale_table(scale, device) -> torch.Tensor:
    if isinstance(scale, torch.Tensor):
        return scale.detach().to(device=device, dtype=torch.float32).reshape(1, 1)
    return torch.full((1, 1), float(scale), dtype=torch.float32, device=device)


def _check_out_dtype(out_dtype):
    if out_dtype not in _OUT_DTYPES:
        raise TypeError(f"kvq: out_dtype must be one of {_OUT_DTYPES}, got {out_dtype}")


def dequantize_int8_per_tensor(q: torch.Tensor, scale: torch.Tensor, out_dtype: torch.dtype) -> torch.Tensor:
    """``(float(q) * float(scale)).to(out_dtype)`` (reference ops.py:68-90). ``scale`` stays on
    the device: no ``float(scale)`` sync."""
    _lib.require_gpu(q, "q")
    _check_out_dtype(out_dtype)
    if q.dtype != torch.int8:
        raise TypeError("q must be int8")
    q = q.contiguous()
    out = torch.empty(q.shape, dtype=out_dtype, device=q.device)
    if q.numel() == 0:
        return out
    D = q.size(-1) if q.dim() else 1
    kernels.dequant_tokens(q.view(1, 1, -1, 1, D), _scale_table(scale, q.device), out.view(1, 1, -1, 1, D), "int8")
    return out


def dequantize_int4_per_tensor_packed(packed: torch.Tensor, scale: torch.Tensor, orig_last_dim: int,
                                      out_dtype: torch.dtype) -> torch.Tensor:
    """Unpack (high nibble first), subtract 8, scale, cast; the pad column of an odd
    ``orig_last_dim`` is dropped (reference ops.py:93-133)."""
    _lib.require_gpu(packed, "packed")
    _check_out_dtype(out_dtype)
    if packed.dtype != torch.uint8:
        raise TypeError("packed must be uint8")
    D = int(orig_last_dim)
    if packed.dim() < 1 or packed.size(-1) != (D + 1) // 2:
        raise ValueError(f"packed last dim {tuple(packed.shape)} does not match orig_last_dim {D}")
    packed = packed.contiguous()
    out = torch.empty(tuple(packed.shape[:-1]) + (D,), dtype=out_dtype, device=packed.device)
    if out.numel() == 0:
        return out
    kernels.dequant_tokens(packed.view(1, 1, -1, 1, packed.size(-1)), _scale_table(scale, packed.device),
                           out.view(1, 1, -1, 1, D), "int4")
    return out


# ----------------------------------------------------------------------------- persistent store


def _skewed_capacity(n: int) -> int:
    """The smallest capacity >= n that is 8 more than a multiple of 16 tokens. A store's (batch row, kv head) rows are
    ``Tcap * Dq`` bytes apart; the attention kernels' waves walk 64 of those rows in lockstep at the same relative offset, and the
    memory controller's channel choice repeats with the row stride: measured on decode attention over a Llama-3-8B batch-8
    store of 16,384 tokens (profiles/r04h_attn_store_capacity_skew.txt), a power-of-two Tcap (2 MiB INT8 rows) takes 39.5 us per
    layer call, Tcap = 16384 + 8 (rows 1 KiB further apart) 38.5, + 64 43.4, + 128 41.4 — every capacity that is 8 mod 16 tokens
    measured 38.5-38.7, every multiple of 64 beyond the power of two 39.6-43.4. Quantise and dequantise do not care
    (profiles/r04a_quant_stride_table.md)."""
    if os.environ.get("KVQ_STORE_CAP_EXACT"):  # measurement knob: the capacity as asked for (the sweep behind the numbers above)
        return n
    return (n + 7) // 16 * 16 + 8


class _KVStore:
    """One quantised KV set in HBM: ``q [G,B,H,Tcap,Dq]`` + stored scales ``[G,Tcap]`` (fp32 view
    of the input-dtype value). G groups never share scales (layer x K|V); all groups hold the
    same number of tokens when driven through QuantizedKVCache, but each keeps its own length so
    that ``layers[i].append`` keeps working."""

    def __init__(self, kind: str, n_groups: int, device, eps: float = 1e-8):
        self.kind = kind
        self.G = int(n_groups)
        self.device = device
        self.eps = eps
        self.lens: List[int] = [0] * self.G
        self.q: Optional[torch.Tensor] = None
        self.scales: Optional[torch.Tensor] = None
        self.ws: Optional[torch.Tensor] = None
        self.cap = 0
        self.B = self.H = self.D = None
        self.in_dtype: Optional[torch.dtype] = None
        self._want = 0  # capacity requested before the first append fixed B, H, D
        # persistent dequantised staging (scope row N1): [G,B,H,cap,D] in the compute dtype; tokens
        # [0, staged) of every group are already dequantised, so a decode step only adds the new one
        self.stage: Optional[torch.Tensor] = None
        self.staged = 0

    # -- allocation ---------------------------------------------------------------------------
    def reserve(self, T: int) -> None:
        """Grow capacity to >= T tokens (amortised doubling; existing tokens are preserved)."""
        if self.B is None or T <= self.cap:
            self._want = max(self._want, T)
            return
        new_cap = _skewed_capacity(max(T, 2 * self.cap, 16))
        Dq = packed_dim(self.kind, self.D)
        q = torch.empty(self.G, self.B, self.H, new_cap, Dq, dtype=QDTYPE[self.kind], device=self.device)
        sc = torch.zeros(self.G, new_cap, dtype=torch.float32, device=self.device)
        used = max(self.lens)
        if self.q is not None and used:
            q[:, :, :, :used] = self.q[:, :, :, :used]
            sc[:, :used] = self.scales[:, :used]
        self.q, self.scales, self.cap = q, sc, new_cap
        if self.stage is not None:  # keep what is already dequantised
            st = torch.empty(self.G, self.B, self.H, new_cap, self.D, dtype=self.stage.dtype, device=self.device)
            if self.staged:
                st[:, :, :, :self.staged] = self.stage[:, :, :, :self.staged]
            self.stage = st

    def _bind(self, x: torch.Tensor) -> None:
        B, H, _, D = x.shape
        if self.B is None:
            self.B, self.H, self.D, self.in_dtype = B, H, D, x.dtype
            self.reserve(max(self._want, 1))
        elif (B, H, D) != (self.B, self.H, self.D) or x.dtype != self.in_dtype:
            raise ValueError(
                f"kvq: KV slice {tuple(x.shape)} {x.dtype} does not match the cache "
                f"[B={self.B},H={self.H},D={self.D}] {self.in_dtype}")

    def _workspace(self, n: int) -> torch.Tensor:
        if self.ws is None or self.ws.numel() < n:
            self.ws = torch.empty(max(n, 1024), dtype=torch.float32, device=self.device)
        return self.ws

    # -- quantise -----------------------------------------------------------------------------
    def append(self, xs: Sequence[torch.Tensor], g0: int = 0) -> None:
        """Quantise ``xs`` (one [B,H,Tn,D] tensor per group g0..g0+len) and append Tn tokens to
        each of those groups: ONE launch. All of them must currently hold the same length."""
        if isinstance(xs, torch.Tensor):  # one [n,B,H,Tn,D] view (e.g. a window of the staging buffer)
            n = xs.size(0)
            first = xs[0]
        else:
            xs = list(xs)
            n = len(xs)
            first = xs[0]
        self._bind(first)
        Tn = first.size(2)
        if Tn == 0:
            return
        t0 = self.lens[g0]
        if any(self.lens[g0 + i] != t0 for i in range(n)):
            raise ValueError("kvq: groups appended together must hold the same number of tokens")
        self.reserve(t0 + Tn)
        qwin = self.q[g0:g0 + n, :, :, t0:t0 + Tn]
        swin = self.scales[g0:g0 + n, t0:t0 + Tn]
        kernels.quant_tokens(xs, qwin, swin, self._workspace(n * Tn), self.kind, self.eps)
        for i in range(n):
            self.lens[g0 + i] = t0 + Tn

    # -- dequantise ---------------------------------------------------------------------------
    def dequant(self, out_dtype: torch.dtype, g0: int = 0, n: Optional[int] = None,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Dequantise groups g0..g0+n (all tokens) into ``[n,B,H,T,D]``: ONE launch."""
        n = self.G - g0 if n is None else n
        T = self.lens[g0]
        if T == 0 or self.q is None:
            raise ValueError("Empty cache")  # reference ops.py:219-220
        if any(self.lens[g0 + i] != T for i in range(n)):
            raise ValueError("kvq: groups dequantised together must hold the same number of tokens")
        if out is None:
            out = torch.empty(n, self.B, self.H, T, self.D, dtype=out_dtype, device=self.device)
        kernels.dequant_tokens(self.q[g0:g0 + n, :, :, :T], self.scales[g0:g0 + n, :T], out, self.kind)
        return out

    def dequant_staged(self, out_dtype: torch.dtype) -> torch.Tensor:
        """All groups, all tokens, as a VIEW ``[G,B,H,T,D]`` of the persistent staging buffer:
        only tokens appended since the last call are dequantised (one launch, O(new tokens)
        instead of the reference's O(T) re-dequantise + T-way cat per step, ops.py:213-269).
        Values are identical to :meth:`dequant`. Earlier views stay valid: staged tokens are
        never rewritten."""
        T = self.lens[0]
        if T == 0 or self.q is None:
            raise ValueError("Empty cache")
        if any(n != T for n in self.lens):
            raise ValueError("kvq: groups dequantised together must hold the same number of tokens")
        if self.stage is None or self.stage.dtype != out_dtype:
            self.stage = torch.empty(self.G, self.B, self.H, self.cap, self.D, dtype=out_dtype, device=self.device)
            self.staged = 0
        if self.staged < T:
            s0 = self.staged
            kernels.dequant_tokens(self.q[:, :, :, s0:T], self.scales[:, s0:T], self.stage[:, :, :, s0:T], self.kind)
            self.staged = T
        return self.stage[:, :, :, :T]

    # -- eviction inside the store ------------------------------------------------------------
    def uniform_len(self) -> int:
        """The token count every group holds; ValueError when they differ (the eviction calls move all groups at once)."""
        T = self.lens[0] if self.lens else 0
        if any(n != T for n in self.lens):
            raise ValueError("kvq: all groups of a store must hold the same number of tokens")
        return T

    def _fresh(self, need: int):
        """New ``q`` / ``scales`` for an out-of-place eviction: the store's own capacity (a ``reserve()`` made for a decode
        loop still holds), more only when ``need`` tokens do not fit (an index list with duplicates)."""
        cap = self.cap if need <= self.cap else _skewed_capacity(need)
        q = torch.empty(self.G, self.B, self.H, cap, packed_dim(self.kind, self.D), dtype=QDTYPE[self.kind], device=self.device)
        sc = torch.zeros(self.G, cap, dtype=torch.float32, device=self.device)
        return q, sc, cap

    def _swap(self, q: torch.Tensor, sc: torch.Tensor, cap: int, T: int) -> None:
        self.q, self.scales = q, sc
        if cap != self.cap:
            self.cap, self.stage = cap, None
        self.lens[:] = [T] * self.G
        self.staged = 0  # the incremental staging view re-dequantises

    def gather(self, idx_dev: torch.Tensor, n: int) -> None:
        """Keep tokens ``idx_dev`` (int32, on the device; ``n`` of them): a row gather of the codes and an element gather of
        the scale table, both through kvq_gather_tokens and both lossless. Code rows travel as 2-byte elements (16 to 256
        bytes per row: gather_rows_k for every head dim the fast paths take); a row of an odd number of bytes is staged
        through an even-sized copy, since the entry point moves 2-byte units. The scale table goes as ``[G,1,1,T,1]``
        4-byte elements."""
        T = self.uniform_len()
        q, sc, cap = self._fresh(n)
        src, dst = self.q[:, :, :, :T], q[:, :, :, :n]
        Dq = src.size(4)
        if Dq % 2 == 0:
            kernels.gather_tokens(src.view(torch.int16), dst.view(torch.int16), idx_dev)
        else:
            pad_in = torch.zeros(self.G, self.B, self.H, T, Dq + 1, dtype=src.dtype, device=self.device)
            pad_in[..., :Dq] = src
            pad_out = torch.empty(self.G, self.B, self.H, n, Dq + 1, dtype=src.dtype, device=self.device)
            kernels.gather_tokens(pad_in.view(torch.int16), pad_out.view(torch.int16), idx_dev)
            dst.copy_(pad_out[..., :Dq])
        kernels.gather_tokens(self.scales[:, :T].unflatten(1, (1, 1, T, 1)), sc[:, :n].unflatten(1, (1, 1, n, 1)), idx_dev)
        self._swap(q, sc, cap, n)

    def chunk_pool(self, chunk_size: int, keep_last: int, dtype: torch.dtype, layers_per_pass: int = 4) -> None:
        """chunk_summarize_kv of the store itself, out of place. One kvq_store_chunk_pool launch where a token slice has at
        most 8,192 elements; larger slices run the composition the library names, ``layers_per_pass`` groups at a time (the
        fp16 staging stays that small): dequantise the old tokens, kvq_chunk_meanpool, quantise the pooled rows only; the
        kept tail's codes and scale words are copied raw. Same bits either way."""
        T = self.uniform_len()
        keep = min(int(keep_last), T)
        old = T - keep
        Tout = kernels.chunk_summary_len(T, chunk_size, keep_last)
        q, sc, cap = self._fresh(Tout)
        if self.B * self.H * self.D <= kernels.STORE_POOL_MAX_SLICE:
            kernels.store_chunk_pool(self.q[:, :, :, :T], self.scales[:, :T], q[:, :, :, :Tout], sc[:, :Tout], self.kind, self.D,
                                     dtype, chunk_size, keep_last, self.eps)
        else:
            n = Tout - keep
            for g0 in range(0, self.G, layers_per_pass):
                gn = min(layers_per_pass, self.G - g0)
                x = torch.empty(gn, self.B, self.H, old, self.D, dtype=dtype, device=self.device)
                kernels.dequant_tokens(self.q[g0:g0 + gn, :, :, :old], self.scales[g0:g0 + gn, :old], x, self.kind)
                pooled = torch.empty(gn, self.B, self.H, n, self.D, dtype=dtype, device=self.device)
                kernels.chunk_meanpool(x, pooled, chunk_size, 0)
                kernels.quant_tokens(pooled, q[g0:g0 + gn, :, :, :n], sc[g0:g0 + gn, :n], self._workspace(gn * n), self.kind, self.eps)
            if keep:
                q[:, :, :, n:Tout] = self.q[:, :, :, old:T]
                sc[:, n:Tout] = self.scales[:, old:T]
        self._swap(q, sc, cap, Tout)

    # -- accounting ---------------------------------------------------------------------------
    def stored_bytes(self, g: int) -> int:
        """numel*itemsize of stored slices + scales, scale itemsize = input dtype's
        (what the reference's lists would hold: ops.py:271-290)."""
        if self.B is None:
            return 0
        T = self.lens[g]
        return T * (self.B * self.H * packed_dim(self.kind, self.D) + self.in_dtype.itemsize)


_MODE_KINDS = {"int8": ("int8", "int8"), "int4": ("int4", "int4"), "mixed": ("int8", "int4")}


class QuantizedLayerKV:
    """Quantised KV cache of one transformer layer (reference ops.py:136-290).

    Modes: ``"int8"`` (K, V int8), ``"int4"`` (both packed int4), ``"mixed"`` (K int8, V int4 —
    reference ops.py:201-210).
    """

    def __init__(self, mode: str = "int8", device: str = "cuda", compute_dtype: torch.dtype = torch.float16,
                 _stores: Optional[Tuple[_KVStore, _KVStore]] = None, _group: int = 0):
        assert mode in ["int8", "int4", "mixed"], f"Invalid mode: {mode}"
        self.mode = mode
        self.device = device
        self.compute_dtype = compute_dtype
        kk, vk = _MODE_KINDS[mode]
        if _stores is None:
            _stores = (_KVStore(kk, 1, device), _KVStore(vk, 1, device))
        self._k, self._v = _stores
        self._g = _group

    def __len__(self) -> int:
        return self._k.lens[self._g]

    @torch.no_grad()
    def append(self, k_1tok: torch.Tensor, v_1tok: torch.Tensor) -> None:
        """Append key/value slices ``[B, H, 1, D]`` (any number of tokens ``[B,H,n,D]`` is accepted:
        each token still gets its own scale, as n single-token appends would)."""
        self._k.append([k_1tok], self._g)
        self._v.append([v_1tok], self._g)

    @torch.no_grad()
    def get_kv(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """Full dequantised ``(K, V)``, each ``[B, H, T, D]`` in ``compute_dtype``."""
        if len(self) == 0:
            raise ValueError("Empty cache")
        k = self._k.dequant(self.compute_dtype, self._g, 1)[0]
        v = self._v.dequant(self.compute_dtype, self._g, 1)[0]
        return k, v

    def estimated_bytes(self) -> int:
        """Bytes of the quantised stores + scales (reference ops.py:271-290)."""
        return self._k.stored_bytes(self._g) + self._v.stored_bytes(self._g)

    # -- the reference's list attributes, materialised on demand as views ------------------------
    def _slices(self, st: _KVStore):
        T = st.lens[self._g]
        return [st.q[self._g, :, :, t:t + 1] for t in range(T)] if st.q is not None else []

    def _scale_list(self, st: _KVStore):
        T = st.lens[self._g]
        if st.scales is None:
            return []
        s = st.scales[self._g, :T].to(st.in_dtype)
        return [s[t] for t in range(T)]

    @property
    def k_store(self):
        return self._slices(self._k)

    @property
    def v_store(self):
        return self._slices(self._v)

    @property
    def k_scales(self):
        return self._scale_list(self._k)

    @property
    def v_scales(self):
        return self._scale_list(self._v)

    @property
    def k_meta(self):
        return [self._k.D if self._k.kind == "int4" else None] * len(self)

    @property
    def v_meta(self):
        return [self._v.D if self._v.kind == "int4" else None] * len(self)


class QuantizedKVCache:
    """Multi-layer quantised KV cache (reference ops.py:293-363): all layers of K share one HBM
    buffer and one launch, likewise V."""

    def __init__(self, n_layers: int, mode: str = "int8", device: str = "cuda",
                 compute_dtype: torch.dtype = torch.float16, incremental: bool = True):
        assert mode in ["int8", "int4", "mixed"], f"Invalid mode: {mode}"
        self.incremental = incremental
        self.mode = mode
        self.device = device
        self.compute_dtype = compute_dtype
        kk, vk = _MODE_KINDS[mode]
        self._k = _KVStore(kk, n_layers, device)
        self._v = _KVStore(vk, n_layers, device)
        self.layers = [
            QuantizedLayerKV(mode=mode, device=device, compute_dtype=compute_dtype,
                             _stores=(self._k, self._v), _group=i)
            for i in range(n_layers)
        ]

    def reserve(self, n_tokens: int) -> None:
        """Pre-size the stores (e.g. prompt + max_new_tokens) so decode never reallocates."""
        self._k.reserve(n_tokens)
        self._v.reserve(n_tokens)

    def _check_layers(self, past_key_values) -> None:
        if len(past_key_values) != len(self.layers):
            raise ValueError(f"kvq: got {len(past_key_values)} layers, cache has {len(self.layers)}")

    @torch.no_grad()
    def append_from_past(self, past_key_values: tuple) -> None:
        """Quantise and append the LAST token of every layer's ``(k, v)`` (reference ops.py:323-330):
        two launches (K set, V set) instead of 2L."""
        self._check_layers(past_key_values)
        self._k.append([k[:, :, -1:, :] for k, _ in past_key_values])
        self._v.append([v[:, :, -1:, :] for _, v in past_key_values])

    @torch.no_grad()
    def init_from_prompt_past(self, past_key_values: tuple) -> None:
        """Quantise every prompt token of every layer, one scale per (layer, K|V, token)
        (reference ops.py:333-342 loops L*T times): two launches."""
        self._check_layers(past_key_values)
        self._k.append([k for k, _ in past_key_values])
        self._v.append([v for _, v in past_key_values])

    @torch.no_grad()
    def to_past_key_values(self, copy: bool = False) -> tuple:
        """Dequantise to the legacy tuple ``tuple_L[(K, V)]``, each ``[B,H,T,D]`` in compute_dtype
        (reference ops.py:345-355): two launches. With ``incremental=True`` (default) the tuple
        holds VIEWS of two persistent staging buffers and only tokens appended since the previous
        call are dequantised — read-only by contract: writing into them corrupts every later step,
        which the reference's fresh tensors (ops.py:267-269) would not. ``copy=True`` (or
        ``incremental=False`` on the cache) re-dequantises everything into fresh buffers the caller
        owns, as the reference does. Same values either way."""
        if not self.layers:
            return tuple()
        if not copy and self.incremental and len(set(self._k.lens)) == 1 and len(set(self._v.lens)) == 1:
            # persistent staging: dequantise only what was appended since the last call
            k = self._k.dequant_staged(self.compute_dtype)
            v = self._v.dequant_staged(self.compute_dtype)
        else:
            k = self._k.dequant(self.compute_dtype)
            v = self._v.dequant(self.compute_dtype)
        return tuple((k[i], v[i]) for i in range(len(self.layers)))

    @torch.no_grad()
    def attend(self, layer: int, q: torch.Tensor, k_new: Optional[torch.Tensor] = None,
               v_new: Optional[torch.Tensor] = None, sm_scale: Optional[float] = None,
               append: bool = False, window: Optional[int] = None, kv_start: Optional[torch.Tensor] = None,
               softcap: float = 0.0, sinks: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Single-token attention of ``layer`` straight from the quantised store (no dequantised copy):
        ``softmax(q K^T * sm_scale) V`` over every stored token, plus the exact ``k_new`` / ``v_new``
        ``[B, Hkv, D]`` as one more token when given — what ``to_past_key_values()`` followed by the
        model's attention computes (reference ops.py:345-355, benchmarker.py:470-471), within fp16
        tolerance. ``q`` is ``[B, Hq, D]`` fp16 / bf16 (Hq a multiple of the cache's kv heads). With
        ``append=True`` the new token is also quantised into the store (``append_from_past`` for this
        layer, ops.py:323-330) by the same call. ``window``: HF's sliding window of that many keys (None = every
        stored token): the query sees only the last ``window`` tokens, its own (the new one, or the last stored one
        without ``k_new``) included; the store still keeps every token. ``kv_start``: int32 ``[B]`` GPU tensor of a
        left-padded batch: row ``b``'s keys before ``kv_start[b]`` are padding (never read); what is stored is unchanged.
        ``softcap`` > 0: every scaled score ``s`` becomes ``softcap * tanh(s / softcap)`` (Gemma 2); ``sinks``: fp32 ``[Hq]``
        GPU tensor, one more softmax term per query head without a value row (gpt-oss). ``0.0`` / ``None`` = none.
        A ``kv_start`` the caller holds refers to CURRENT store positions: after an eviction it is the caller's to remap."""
        window = kernels._window_arg(0 if window is None else window, "attend")
        k, v = self._k, self._v
        T = k.lens[layer]
        if T != v.lens[layer] or k.q is None:
            raise ValueError("Empty cache")
        if append and (k_new is None or v_new is None):
            raise ValueError("kvq: append=True needs k_new and v_new")
        if q.dim() != 3:
            raise ValueError(f"kvq: attend takes a [B, Hq, D] query, got {tuple(q.shape)}")
        B, Hq, D = q.shape
        if append:
            # an appended token must be what append_from_past would have been given: the store's own
            # input dtype (the scale is rounded to it, estimated_bytes counts its itemsize) and shape
            for name, t in (("k_new", k_new), ("v_new", v_new)):
                if t.dtype != k.in_dtype or tuple(t.shape) != (k.B, k.H, k.D):
                    raise ValueError(f"kvq: attend(append=True) {name} {tuple(t.shape)} {t.dtype} does not match the cache "
                                     f"[B={k.B},H={k.H},D={k.D}] {k.in_dtype}")
            k.reserve(T + 1)
            v.reserve(T + 1)
        scale = float(sm_scale) if sm_scale is not None else D ** -0.5
        out = torch.empty_like(q)
        # the workspace size (a host loop over the capacity) and the per-layer plans are looked up only when
        # the shape, the capacity or the store allocation changes — not once per call
        ws_key = (B, Hq, D, q.dtype, k.cap, q.device)
        if getattr(self, "_attn_ws_key", None) != ws_key:
            need = kernels.decode_attn_workspace_cap(B, Hq, k.H, max(k.cap, T + 1), D)
            if getattr(self, "_attn_ws", None) is None or self._attn_ws.numel() < need or self._attn_ws.device != q.device:
                self._attn_ws = torch.empty(need, dtype=torch.float32, device=q.device)
            self._attn_ws_key = ws_key
            self._attn_plans = {}
        if append:
            pkey = (k.q.data_ptr(), v.q.data_ptr(), q.dtype, B, Hq, D)
            plan = self._attn_plans.get(layer)
            if plan is None or plan.key[:2] != (k.q[layer].data_ptr(), v.q[layer].data_ptr()) or plan.key[2:] != pkey[2:]:
                plan = self._attn_plans[layer] = kernels.DecodeStepPlan(q, k.q[layer], k.scales[layer], k.kind, v.q[layer],
                                                                        v.scales[layer], v.kind, k.eps)
            kernels.decode_step(plan, q, k_new, v_new, T, out, self._attn_ws, scale, window, kv_start, softcap, sinks)
            k.lens[layer] = v.lens[layer] = T + 1
        else:
            kernels.decode_attn(q, k.q[layer], k.scales[layer], k.kind, v.q[layer], v.scales[layer], v.kind, T, out,
                                self._attn_ws, scale, k_new, v_new, window, kv_start, softcap, sinks)
        return out

    @torch.no_grad()
    def extend(self, layer: int, q: torch.Tensor, k_new: torch.Tensor, v_new: torch.Tensor,
               sm_scale: Optional[float] = None, append: bool = True, window: Optional[int] = None,
               kv_start: Optional[torch.Tensor] = None, softcap: float = 0.0,
               sinks: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Multi-token causal attention of ``layer`` straight from the quantised store: ``q`` ``[B, Hq, S, D]``
        attends every stored token and, causally, the chunk's exact ``k_new`` / ``v_new`` ``[B, Hkv, S, D]``
        (query ``s`` sees chunk tokens ``j <= s``) — what ``to_past_key_values()`` followed by the model's
        attention with HF's causal mask computes for a forward of ``S`` tokens (chunked prefill, the next turn of
        a chat, a speculative-decoding verify), within fp16 / bf16 tolerance. The store may be empty (plain
        causal attention over the chunk). With ``append=True`` the chunk is then quantised into this layer's K
        and V groups, the same bytes ``init_from_prompt_past`` would write for those tokens. Returns
        ``[B, Hq, S, D]`` in ``q``'s dtype (contiguous). ``window``: HF's sliding window of that many keys (None =
        none): query ``s`` (position ``T + s``) sees the tokens at positions ``> T + s - window`` only. ``kv_start``:
        int32 ``[B]`` GPU tensor of a left-padded batch: row ``b`` sees no key before ``kv_start[b]``; a query whose own
        position is padding gets zeros. The chunk is stored whole either way. ``softcap`` / ``sinks``: as for
        :meth:`attend`; the cap applies to stored and chunk scores alike. A ``kv_start`` the caller holds refers to CURRENT
        store positions: after an eviction it is the caller's to remap."""
        window = kernels._window_arg(0 if window is None else window, "extend")
        k, v = self._k, self._v
        if not 0 <= layer < len(self.layers):
            raise IndexError(f"kvq: layer {layer} out of range ({len(self.layers)} layers)")
        T = k.lens[layer]
        if T != v.lens[layer]:
            raise ValueError("kvq: the layer's K and V stores hold different token counts")
        if q.dim() != 4 or k_new.dim() != 4 or v_new.dim() != 4:
            raise ValueError(f"kvq: extend takes [B, Hq, S, D] / [B, Hkv, S, D] tensors, got {tuple(q.shape)} / "
                             f"{tuple(k_new.shape)} / {tuple(v_new.shape)}")
        B, Hq, S, D = q.shape
        if k.B is not None:
            for name, t in (("k_new", k_new), ("v_new", v_new)):
                if (t.size(0), t.size(1), t.size(3)) != (k.B, k.H, k.D) or (append and t.dtype != k.in_dtype):
                    raise ValueError(f"kvq: extend {name} {tuple(t.shape)} {t.dtype} does not match the cache "
                                     f"[B={k.B},H={k.H},D={k.D}] {k.in_dtype}")
        if append:
            # bind / grow the stores before the call: an empty store gets its shape from the chunk
            k._bind(k_new)
            v._bind(v_new)
            k.reserve(T + S)
            v.reserve(T + S)
        if k.q is None or v.q is None:
            raise ValueError("kvq: extend(append=False) on a cache that has never been bound to a shape")
        scale = float(sm_scale) if sm_scale is not None else D ** -0.5
        out = torch.empty_like(q, memory_format=torch.contiguous_format)
        # one workspace, sized at the reserved capacity (the size is non-decreasing in the stored-token count)
        need = kernels.extend_attn_workspace(B, Hq, k.H, max(k.cap, T), S, D)
        ws = getattr(self, "_ext_ws", None)
        if ws is None or ws.numel() < max(need, 1) or ws.device != q.device:
            ws = self._ext_ws = torch.empty(max(need, 1), dtype=torch.float32, device=q.device)
        kernels.extend_attn(q, k.q[layer], k.scales[layer], k.kind, v.q[layer], v.scales[layer], v.kind, T,
                            k_new, v_new, out, ws, scale, window, kv_start, softcap, sinks)
        if append:
            k.append([k_new], layer)
            v.append([v_new], layer)
        return out

    # -- eviction inside the quantised store --------------------------------------------------------
    # keep_tokens / trim / chunk_summarize are OUT OF PLACE: the result is written into freshly allocated code and scale
    # tensors of the store's capacity, which are then swapped in. Transient memory: one more store.

    def _refuse_left_padded(self, what: str, why: str) -> None:
        owner = self._fused_owner() if getattr(self, "_fused_owner", None) is not None else None
        if owner is not None and getattr(owner, "kv_start", None) is not None:
            raise RuntimeError(f"kvq: {what} on a left-padded batch (FusedQuantizedCache.set_left_padding was called): {why}")

    def _evictable_len(self) -> int:
        owner = self._fused_owner() if getattr(self, "_fused_owner", None) is not None else None
        if owner is not None and owner.t_dev is not None:
            raise RuntimeError("kvq: the cache is driven by a captured decode graph (FusedQuantizedCache.t_dev is set): the graph "
                               "holds the store's pointers, eviction would replace them")
        self._refuse_left_padded("eviction", "the per-row key starts are positions in the un-evicted store, and the cache keeps "
                                 "them for its life: after a compaction they would hide real tokens, a pooled summary would "
                                 "mix a row's padding slots into its real ones")
        staged = self._staged_owner() if getattr(self, "_staged_owner", None) is not None else None
        if staged is not None and staged.in_flight():
            raise RuntimeError("kvq: a StagedQuantizedCache forward is in flight (sync() without commit()): commit first")
        T = self._k.uniform_len()
        if T != self._v.uniform_len():
            raise ValueError("kvq: the K and V stores hold different token counts")
        if T == 0 or self._k.q is None:
            raise ValueError("Empty cache")
        return T

    def _after_eviction(self) -> None:
        self._attn_plans = {}  # they hold the old stores' pointers
        self._score_ws_key = None  # key_scores sizes its workspace again
        owner = self._fused_owner() if getattr(self, "_fused_owner", None) is not None else None
        if owner is not None:
            for layer in owner.cache.layers:
                layer.plan = None

    @torch.no_grad()
    def keep_tokens(self, idx) -> None:
        """Keep exactly the stored tokens ``idx``, in that order (duplicates allowed), in every layer's K and V: afterwards
        token ``j`` holds the raw code bytes and the raw scale word of the former token ``idx[j]``, so
        ``to_past_key_values(copy=True)`` is bit for bit ``index_select`` of what it was. ``idx``: a list of ints (validated
        against ``[0, T)``, ValueError), or an int32 / int64 tensor; a GPU tensor is used as is, without a host
        synchronisation: an out-of-range entry then gives a row of zero codes with a zero scale, as kvq_gather_tokens
        documents. An empty ``idx`` raises ValueError. Out of place: transient memory is one more store; the capacity is
        kept. A ``kv_start`` the caller passes to :meth:`attend` / :meth:`extend` refers to current store positions and is the
        caller's to remap afterwards; a FusedQuantizedCache that keeps one itself (``set_left_padding``) makes every eviction
        and :meth:`key_scores` raise RuntimeError."""
        T = self._evictable_len()
        if isinstance(idx, torch.Tensor):
            if idx.dtype not in (torch.int32, torch.int64) or idx.dim() != 1:
                raise ValueError(f"kvq: keep_tokens takes a 1-D int32 / int64 index tensor, got {idx.dtype} {tuple(idx.shape)}")
            if not idx.is_cuda:
                idx = idx.tolist()
        if isinstance(idx, torch.Tensor):
            n = idx.numel()
            if n == 0:
                raise ValueError("kvq: keep_tokens needs at least one token")
            idx_dev = idx.to(device=self._k.q.device, dtype=torch.int32).contiguous()
        else:
            idx = [int(i) for i in idx]
            n = len(idx)
            if n == 0:
                raise ValueError("kvq: keep_tokens needs at least one token")
            if min(idx) < 0 or max(idx) >= T:
                raise ValueError(f"kvq: keep_tokens index out of range [0, {T})")
            idx_dev = torch.tensor(idx, dtype=torch.int32).to(self._k.q.device, non_blocking=True)
        self._k.gather(idx_dev, n)
        self._v.gather(idx_dev, n)
        self._after_eviction()

    @torch.no_grad()
    def trim(self, policy: str, *args, **kwargs) -> None:
        """Apply an index-select eviction policy to the store itself: ``"sliding_window"``, ``"prefix_window"``,
        ``"strided"``, ``"block_old"`` or ``"budget_old"`` with the arguments (names, order, defaults) of the
        ``trim_kv_<policy>`` function, from the same index functions. Lossless: see :meth:`keep_tokens`. A policy that keeps
        everything does nothing (no launch, no reallocation)."""
        fn = KEEP_INDEX_FNS.get(policy)
        if fn is None:
            raise ValueError(f"kvq: unknown eviction policy {policy!r} (one of {sorted(KEEP_INDEX_FNS)})")
        if "device" in kwargs:
            raise TypeError("kvq: trim() takes the policy's own arguments only")
        for name, v in list(zip(fn.__code__.co_varnames[1:], args)) + list(kwargs.items()):
            if isinstance(v, bool) or not isinstance(v, int):
                raise TypeError(f"kvq: trim({policy!r}) argument {name} must be an int, got {v!r}")
            if v < 0:
                raise ValueError(f"kvq: trim({policy!r}) argument {name} must be >= 0, got {v}")
        T = self._evictable_len()
        try:
            keep = fn(T, *args, device=self._k.q.device, **kwargs)
        except AssertionError as e:
            raise ValueError(f"kvq: trim({policy!r}): bad policy arguments") from e
        if keep is not None:
            self.keep_tokens(keep)

    @torch.no_grad()
    def chunk_summarize(self, chunk_size: int, keep_last: int) -> None:
        """``chunk_summarize_kv`` inside the quantised domain: tokens older than the last ``keep_last`` become requantised
        mean-pooled summaries of ``chunk_size`` tokens, the last ``keep_last`` keep their codes and scales untouched.
        Bit for bit dequantise -> ``chunk_summarize_kv`` -> quantise of the pooled rows; one kvq_store_chunk_pool launch per
        store (K set, V set), or that composition a few layers at a time where a token slice exceeds 8,192 elements.
        Requires the store's input dtype to be ``compute_dtype`` (ValueError). Nothing to compress: nothing happens. Out
        of place: transient memory is one more store; the capacity is kept."""
        if isinstance(chunk_size, bool) or isinstance(keep_last, bool) or int(chunk_size) != chunk_size or int(keep_last) != keep_last:
            raise TypeError("kvq: chunk_summarize takes integers")
        if chunk_size <= 0 or keep_last < 0:
            raise ValueError("kvq: chunk_size must be > 0 and keep_last >= 0")
        T = self._evictable_len()
        for st in (self._k, self._v):
            if st.in_dtype != self.compute_dtype or st.in_dtype not in (torch.float16, torch.bfloat16):
                raise ValueError(f"kvq: chunk_summarize needs a store quantised from compute_dtype fp16 / bf16 (store {st.in_dtype}, "
                                 f"compute_dtype {self.compute_dtype})")
        if T - min(int(keep_last), T) <= 0:
            return
        self._k.chunk_pool(int(chunk_size), int(keep_last), self.compute_dtype)
        self._v.chunk_pool(int(chunk_size), int(keep_last), self.compute_dtype)
        self._after_eviction()

    # -- attention-guided eviction --------------------------------------------------------------------

    @torch.no_grad()
    def key_scores(self, layer: int, q: torch.Tensor, sm_scale: Optional[float] = None, out: Optional[torch.Tensor] = None,
                   accumulate: bool = False) -> torch.Tensor:
        """Attention mass every stored key of ``layer`` receives from ``q``, straight from the quantised store (kvq_key_scores;
        no dequantised copy, no score tensor). ``q``: ``[B, Hq, S, D]`` fp16 / bf16, the queries OF THE LAST ``S`` STORED
        TOKENS (row ``s`` sits at position ``T - S + s`` and sees the keys up to its own), or ``[B, Hq, D]``: the decode query
        whose token has just been appended. Returns fp32 ``[B, Hkv, T]``: per kv head, the softmax probabilities summed over
        the head's query group and over the rows that see the key (``.sum(-1) == (Hq / Hkv) * S``). ``out``: an fp32
        ``[B, Hkv, >= T]`` table to write into (the first ``T`` tokens are returned; the rest is left as it is);
        ``accumulate=True`` adds to what ``out`` holds: H2O's running sum over decode steps, or a sum over layers.
        ``sm_scale`` defaults to ``D ** -0.5``. Bit-identical from run to run."""
        k = self._k
        self._refuse_left_padded("key_scores", "the kernel has no per-row key start, so a row's padding keys would receive "
                                 "attention mass")
        if not 0 <= layer < len(self.layers):
            raise IndexError(f"kvq: layer {layer} out of range ({len(self.layers)} layers)")
        T = k.lens[layer]
        if T == 0 or k.q is None:
            raise ValueError("Empty cache")
        if q.dim() == 3:
            q = q.unsqueeze(2)
        if q.dim() != 4:
            raise ValueError(f"kvq: key_scores takes a [B, Hq, S, D] or [B, Hq, D] query, got {tuple(q.shape)}")
        B, Hq, S, D = q.shape
        if accumulate and out is None:
            raise ValueError("kvq: key_scores(accumulate=True) needs the table to add to (out=)")
        if out is None:
            out = torch.empty(B, k.H, T, dtype=torch.float32, device=q.device)
        scale = float(sm_scale) if sm_scale is not None else D ** -0.5
        # the workspace is sized at the reserved capacity (the size is non-decreasing in the stored-token count) and looked
        # up again only when the shape or the capacity changes, or after an eviction
        ws_key = (B, Hq, S, D, k.cap, q.device)
        if getattr(self, "_score_ws_key", None) != ws_key:
            need = kernels.key_scores_workspace(B, Hq, k.H, max(k.cap, T), S, D)
            if getattr(self, "_score_ws", None) is None or self._score_ws.numel() < need or self._score_ws.device != q.device:
                self._score_ws = torch.empty(need, dtype=torch.float32, device=q.device)
            self._score_ws_key = ws_key
        kernels.key_scores(q, k.q[layer], k.scales[layer], k.kind, T, out, self._score_ws, scale, accumulate)
        return out[:, :, :T]

    @torch.no_grad()
    def evict_by_scores(self, scores: torch.Tensor, budget: int, prefix_len: int = 0, recent: int = 0, pool: int = 1):
        """Keep the ``budget`` stored tokens ``keep_indices_top_scores`` chooses from ``scores`` (any shape ``[..., T]``, e.g.
        what :meth:`key_scores` returns: summed over the leading dims in fp32), in every layer's K and V
        (:meth:`keep_tokens`: lossless, out of place). Returns the kept positions (int32, ascending, on the store's device),
        or ``None`` when everything is kept. No host synchronisation. Refused, like every eviction, while a captured decode
        graph or a staged forward holds the store."""
        T = self._evictable_len()
        if not isinstance(scores, torch.Tensor) or scores.dim() < 1 or scores.size(-1) != T:
            raise ValueError(f"kvq: evict_by_scores takes scores of shape [..., T = {T}]")
        s = scores.detach().to(torch.float32).reshape(-1, T).sum(dim=0)
        keep = keep_indices_top_scores(s, budget, prefix_len, recent, pool, device=self._k.q.device)
        if keep is not None:
            self.keep_tokens(keep)
        return keep

    @torch.no_grad()
    def compress_prompt(self, obs_queries, budget: int, prefix_len: int = 0, pool: int = 1, sm_scale: Optional[float] = None):
        """SnapKV on the store: keep the ``budget`` prompt tokens the last prompt queries attend to. ``obs_queries``: one
        ``[B, Hq, S, D]`` tensor per layer, the queries of the last ``S`` prompt tokens (the observation window, already
        stored). Every layer's :meth:`key_scores` is accumulated into one table, which is reduced over batch rows and kv
        heads and max-pooled over ``pool`` neighbours; the first ``prefix_len`` tokens and the observation window are always
        kept. Returns the kept positions, or ``None`` when everything is kept."""
        T = self._evictable_len()
        if len(obs_queries) != len(self.layers):
            raise ValueError(f"kvq: got {len(obs_queries)} query tensors, cache has {len(self.layers)} layers")
        shapes = {tuple(q.shape) for q in obs_queries}
        if len(shapes) != 1 or len(next(iter(shapes))) != 4:
            raise ValueError(f"kvq: compress_prompt takes one [B, Hq, S, D] query tensor per layer, got {sorted(shapes)}")
        B, _, S, _ = obs_queries[0].shape
        table = torch.empty(B, self._k.H, T, dtype=torch.float32, device=obs_queries[0].device)
        for layer, q in enumerate(obs_queries):
            self.key_scores(layer, q, sm_scale, out=table, accumulate=layer > 0)
        return self.evict_by_scores(table, budget, prefix_len, recent=S, pool=pool)

    def estimated_bytes(self) -> int:
        """Total bytes over layers (reference ops.py:357-363)."""
        return sum(layer.estimated_bytes() for layer in self.layers)
