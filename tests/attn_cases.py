"""Adversarial inputs, an error budget and a float64 model of attention over the quantised store, shared by
tests/test_attn_discrimination.py (CPU: the check rejects wrong answers) and tests/test_gpu_attn_adversarial.py (GPU: the
kernels pass it).

A case is one layer's inputs, built in numpy from a seed and quantised by ``O.quantize_tokens``: decode (one query token,
optionally the exact new token) or extend (an S-token chunk under the lower-right causal mask). Every case carries
POSITIONAL PROBES: query rows whose query is a Hadamard direction that one target token's key carries in the same kv head
(18 nats above everything else), so that the row's output is that token's V. Targets sit at stored tokens 0, 63, 64, T-1,
at both sides of every split boundary, at chunk tokens j = s (diagonal) and j = s + 1 (the future: the row must NOT see
it), and on decode's new token. Adjacent targets alternate key and value amplitudes (x1 / x3, x2 / x6), so that swapping
two tokens' scales moves a probe. The family shapes the remaining rows and tokens:

* ``sink``: token 0 (or, ``variant="chunk"``, chunk token 0) scores 12-20 nats above the rest with a V 100x smaller;
* ``probe``: every row is a probe;
* ``outlier``: channels 3 and D/2 + 5 of q and k at ``factor`` (16 or 100) x the rest;
* ``vrange``: per-token V scales log-uniform over four decades; the rows attend to the smallest-scale tokens, which come
  after the largest-scale ones in walk order (the running / wave V reference scale must not lose them);
* ``late``: scores within -150 .. 0 except for a few tokens at 140 .. 150 in the last stored tile (extend: in the chunk),
  so that every earlier split's merge weight underflows to 0.

``window=W`` (HF's sliding window: a query at position p sees key k iff p - W < k <= p; decode p = T with the new token,
T - 1 without; extend p = T + s) adds probes at each row's LOWER edge: a target at p - W + 1 the row must see and a
forbidden one at p - W it must not (aimed at like the j = s + 1 future probes). The stored probe targets and the
families then live in the VIEW [lo, T), lo = the first stored token any row sees (decode's lo, extend's lo0 = row 0's):
the sink sits at token 0 (outside, it must vanish) or, ``variant="lo"``, at lo (extend: at lo0 + S - 1, the last row's
edge, so that every row sees it); ``late`` puts its hot tokens in the
window's first 64 tokens; ``vrange`` puts the largest V scales at the bottom of the view and the attended smallest at
its top. In extend the edge probes sit on rows chosen to put edges at the first and last rows, around s = W (edges into
the chunk), at the view's 64-token tile boundaries and at split boundaries.

``kv_start=[...]`` (a left-padded batch, DESIGN 3.7: row b of the batch sees key k iff max(start_b, p - W + 1 if W else 0)
<= k <= p; a row that sees no key is zeros) builds the case per batch row (:func:`_make_padded_case`): the stored targets
sit at lo_b + the positions above, lo_b the row's own first visible stored token and the split boundaries those of the
row's own layout (:func:`padded_live`), with an "in" probe at each row's first visible key and an "out" probe at the key
before it; the families' hot spots move to each row's view. ``attend`` and ``bound`` then apply the row's own visibility,
and ``bound`` takes the V-scale maximum from the row's own view. :func:`padded_perturbations` lists the deliberate
mistakes of such a launch. ``kv_start=None`` changes nothing.
"""
import numpy as np

from oracle import kvq_oracle as O

TOL = {"f16": 2e-3, "bf16": 1.6e-2}  # the suite's standard tolerance (tests/test_gpu_attn.py)
P_REL = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}   # unit roundoff of P' in the compute dtype
P_MIN = {"f16": 2.0 ** -14, "bf16": 0.0}         # smallest normal (bf16: fp32's range, never reached here)
P_ABS = {"f16": 2.0 ** -25, "bf16": 0.0}         # half the subnormal spacing
QPLANE = 1.0 / 64516.0                            # two int8 query planes: error <= max|q| / 254^2 per element
EXT_QB, EXT_TC, EXT_MAX_SPLIT, EXT_TARGET_WG = 64, 64, 64, 1024


def extend_plan(B, Hq, Hkv, T, S):
    """Python restatement of extend_plan (csrc/attn/extend.inc): (query blocks, splits, stored tiles per split)."""
    M = S * (Hq // Hkv)
    qbn = (M + EXT_QB - 1) // EXT_QB
    ntiles = (T + EXT_TC - 1) // EXT_TC
    ns = 1
    if ntiles:
        base = qbn * B * Hkv
        ns = max(1, min((EXT_TARGET_WG + base - 1) // base, (ntiles + 1) // 2, EXT_MAX_SPLIT))
    per = (ntiles + ns - 1) // ns if ntiles else 0
    return qbn, ((ntiles + per - 1) // per if ntiles else 1), per


KINDS = ("int8", "int4")  # the headline pair: INT8 keys, INT4 values
BITS = {"int8": 8, "int4": 4}
# decode routes: name -> (B, Hq, Hkv, T, D), tunables, kernel-log prefix, tokens per split
DECODE_ROUTES = {
    "one-tile MFMA": ((2, 32, 8, 600, 128), {"attn_stream_tpw": -1}, "decode_attn_partial_mfma_k<8, 4, 128, 128, false>", (128,)),
    "ring hd128 TG4": ((2, 32, 8, 600, 128), {"attn_stream_tpw": 2}, "decode_attn_lds_mfma_k<8, 4, 64, true, 2, 4, 128, false>", (128,)),
    "ring hd128 TG1": ((2, 16, 2, 600, 128), {"attn_stream_tpw": 3}, "decode_attn_lds_mfma_k<8, 4, 64, true, 2, 1, 128, false>", (192,)),
    "ring hd64": ((2, 32, 8, 600, 64), {"attn_stream_tpw": 2}, "decode_attn_lds_mfma_k<8, 4, 64, true, 2, 4, 64, false>", (128,)),
    "VALU hd32": ((2, 16, 4, 600, 32), {}, "decode_attn_partial_k<8, 4, 4>", (512,)),
    "VALU hd256": ((2, 16, 4, 300, 256), {}, "decode_attn_partial_k<8, 4, 4>", (64,)),
}
EXTEND_ROUTES = {  # name -> (B, Hq, Hkv, T, S, D), expected split count
    "one split": ((1, 32, 8, 128, 16, 128), 1),
    "splits + merge": ((1, 32, 8, 1000, 16, 128), 8),
    "nq 7, splits + merge": ((1, 28, 4, 700, 9, 128), None),
    "head_dim 64, nq 3": ((2, 12, 4, 500, 7, 64), None),
}

# the decode plan's constants (csrc/attn/host.inc, common.inc, merge.inc)
STREAM_TC, MFMA_TC, LDS_SLOTS, MAX_SPLIT, MAX_TS, ATTN_BLOCK, ATTN_UNROLL, MERGE_PF = 64, 128, 1024, 4096, 1024, 256, 4, 16
DEFAULT_TUNABLES = dict(attn_force_valu=0, attn_stream_tpw=0, attn_lds=-1, attn_ring_dev=1, attn_merge_wave=1,
                        attn_merge_fast=1, attn_new_token_parts=1)


class DevPlan:
    """What the library launches for a device-count decode step (kvq_decode_step_dev, no window) planned for ``bound``:
    ``partial`` / ``merge`` the names the kernel log shows, ``by_wave`` the one-wave-per-head form of
    ``decode_attn_merge_fast_k<2, ...>``, ``append`` the routine that quantises the new token (``regs``, ``parts`` or
    ``block``), ``nsplit`` / ``ts`` / ``tpw`` the host's split layout (``tpw`` 0: one-tile splits). :meth:`live` gives
    the split layout the kernels derive from the count."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def live(self, count):
        """(tokens per live split, live split count) at device count ``count`` (clamped to the bound, as live_tokens
        does): the ring's ring_dev_tpw / live_split_tokens, else the host's split size."""
        t = min(max(count, 0), self.bound)
        ts = self.ts
        if self.tpw:
            ntiles = -(-t // STREAM_TC)
            ts = max(1, -(-ntiles // self.nsplit)) * STREAM_TC
        return ts, -(-t // ts)

    def __repr__(self):
        return (f"DevPlan({self.partial!r}, {self.merge!r}{' by wave' if self.by_wave else ''}, append={self.append}, "
                f"nsplit={self.nsplit}, ts={self.ts}, tpw={self.tpw})")


def dev_plan(B, Hq, Hkv, D, k_bits, bound, tunables=None, v_bits=4):
    """Python restatement of the plan of a device-count decode step: use_mfma, use_lds, stream_tpw, plan / plan_onetile and
    the launch choices of launch_partial, launch_merge, decode_attn_impl and new_token_nparts (host.inc), with ``tunables`` over the
    library's defaults. tests/test_gpu_decode_dev_routes.py asserts the kernel log against it."""
    tn = {**DEFAULT_TUNABLES, **(tunables or {})}
    T = bound
    nq = Hq // Hkv
    mfma = D in (128, 64) and 1 <= nq <= 16 and not tn["attn_force_valu"]
    lds = tn["attn_lds"] != 0 and mfma and (D == 128 or (D == 64 and k_bits == 8))
    ring_dev = tn["attn_ring_dev"] != 0
    tpw = 0
    if ring_dev and lds and T > 0 and tn["attn_stream_tpw"] >= 0:  # stream_tpw
        forced = tn["attn_stream_tpw"]
        ntiles = -(-T // STREAM_TC)
        tpw = forced if forced > 0 else -(-(ntiles * B * Hkv) // LDS_SLOTS)
        tpw = 0 if (forced <= 0 and tpw < 3) else min(tpw, ntiles)
        if tpw and -(-T // (tpw * STREAM_TC)) > MAX_SPLIT:
            tpw = 0
    if tpw:
        ts = tpw * STREAM_TC
    elif mfma:  # plan_onetile
        ts = MFMA_TC
    else:
        step = ATTN_BLOCK // (D // 16) * ATTN_UNROLL
        m = max(1, -(-(T * max(1, B * Hkv)) // (step * 4096)))
        ts = m * step
        if ts > MAX_TS or -(-T // ts) > MAX_SPLIT:
            ts = MAX_TS // step * step
    nsplit = -(-T // ts)
    kb, vb = k_bits, v_bits
    if tpw:  # the ring kernel's device-count instantiations
        tg = 4 if (kb == 8 and nq <= 4) else 1
        partial = f"decode_attn_lds_mfma_k<{kb}, {vb}, 64, {'true' if kb == 8 else 'false'}, 2, {tg}, {D}, true>"
    elif mfma:
        partial = f"decode_attn_partial_mfma_k<{kb}, {vb}, {MFMA_TC}, {D}, false>"
    else:
        partial = f"decode_attn_partial_k<{kb}, {vb}, {1 if nq == 1 else 2 if nq == 2 else 4 if nq <= 4 else 8}>"
    n = B * Hkv * D
    nparts = 1 if (n <= 8192 or D not in (128, 64) or not tn["attn_new_token_parts"]) else min(32, -(-n // 8192))
    by_wave = False
    if 1 <= nsplit <= ATTN_BLOCK and D <= ATTN_BLOCK and tn["attn_merge_fast"]:
        rdev = "true" if tpw else "false"
        need = -(-nsplit // (ATTN_BLOCK // (D // 4)))
        by_wave = need <= 2 and D in (128, 64) and nsplit <= 16 and tn["attn_merge_wave"] != 0
        merge = f"decode_attn_merge_fast_k<{2 if need <= 2 else MERGE_PF}, {rdev}>"
        append = "parts" if nparts > 1 else "regs" if n <= 2 * ATTN_BLOCK * 16 else "block"
    else:
        merge = "decode_attn_merge_k"
        append = "parts" if nparts > 1 else "block"
    return DevPlan(partial=partial, merge=merge, by_wave=by_wave, append=append, nsplit=nsplit, ts=ts, tpw=tpw,
                   bound=bound)


def dev_plan_changes(p, lo=1, hi=None):
    """Counts t in [lo, hi] (default: up to the bound) at which the live layout of plan ``p`` differs from t - 1's:
    {t: (tokens per live split, live split count)}."""
    hi = p.bound if hi is None else hi
    out, prev = {}, p.live(lo - 1)
    for t in range(lo, hi + 1):
        cur = p.live(t)
        if cur != prev:
            out[t] = cur
        prev = cur
    return out


def hadamard(n):
    h = np.ones((1, 1))
    while h.shape[0] < n:
        h = np.block([[h, h], [h, -h]])
    return h


def narrow(x, dtype):
    """float -> the compute dtype's representation (fp16 array, bf16 as uint16 bits)."""
    x = np.asarray(x, np.float32)
    return O.f32_to_bf16_bits(x) if dtype == "bf16" else x.astype(np.float16)


def widen(a, dtype):
    return (O.bf16_bits_to_f32(a) if dtype == "bf16" else np.asarray(a, np.float32)).astype(np.float64)


def _codes(qarr, kind, D):
    """integer codes of a [B,H,T,Dq] store as float64 [B,H,T,D] (dequantise with scale 1: exact)."""
    if qarr.shape[2] == 0:
        return np.zeros(qarr.shape[:3] + (D,))
    ones = np.ones((1, qarr.shape[2]), np.float32)
    return O.dequantize_tokens(qarr[None], ones, kind, D, "f16")[0].astype(np.float64)


def view_lo(mode, T, W, with_new=True):
    """First stored token any query row sees under a window of W keys (0: none): decode max(0, p + 1 - W) with p = T
    (new token) or T - 1; extend row 0's, lo0 = max(0, T + 1 - W). The kernels read the store from there on."""
    if not W:
        return 0
    return max(0, T + (1 if (mode == "extend" or with_new) else 0) - W)


def clamp_starts(mode, kv_start, T, S):
    """``kv_start`` clamped as DESIGN 3.7 says: decode to [0, T], extend to [0, T + S]"""
    hi = T + S if mode == "extend" else T
    return [min(max(int(s), 0), hi) for s in kv_start]


def padded_los(mode, T, W, with_new, starts):
    """Each batch row's first visible STORED token under (clamped) starts: the larger of the window's bound (decode's
    lo, extend's lo0) and the start, at most T (padded_lo in csrc/attn/common.inc)."""
    lo = view_lo(mode, T, W, with_new)
    return [max(lo, min(s, T)) for s in starts]


class Case:
    """One layer's inputs. q [B,Hq,S,D]; stored K / V [B,Hkv,T,D] quantised to (kq, ks) / (vq, vs); kn / vn the exact
    new tokens [B,Hkv,S,D] (extend) or [B,Hkv,D] / None (decode). All raw arrays in the compute dtype's representation.
    ``window``: HF's sliding window of that many keys (0: none); ``lo``: the view's first stored token (:func:`view_lo`).
    ``kv_start`` (a left-padded batch): None, or the rows' key starts clamped as the kernels clamp them
    (:func:`clamp_starts`); ``los`` then holds each batch row's first visible stored token (:func:`padded_los`)."""

    def __init__(self, mode, dtype, kinds, sm, q, k, v, kn, vn, info, window=0, kv_start=None):
        self.mode, self.dtype, self.kinds, self.sm, self.info = mode, dtype, kinds, sm, info
        self.window = window
        odt = "bf16" if dtype == "bf16" else None
        self.q, self.kn, self.vn = q, kn, vn
        self.kraw, self.vraw = k, v  # the stored tokens before quantisation
        B, Hkv, T, D = k.shape
        self.B, self.Hkv, self.T, self.D = B, Hkv, T, D
        self.Hq = q.shape[1]
        self.S = q.shape[2] if mode == "extend" else 1
        if T:
            kq, _, ks = O.quantize_tokens(k[None], kinds[0], dtype=odt)
            vq, _, vs = O.quantize_tokens(v[None], kinds[1], dtype=odt)
            self.kq, self.ks, self.vq, self.vs = kq[0], ks[0], vq[0], vs[0]
        else:
            dq = {"int8": (D, np.int8), "int4": (D // 2, np.uint8)}
            self.kq = np.zeros((B, Hkv, 0, dq[kinds[0]][0]), dq[kinds[0]][1])
            self.vq = np.zeros((B, Hkv, 0, dq[kinds[1]][0]), dq[kinds[1]][1])
            self.ks = self.vs = np.zeros(0, np.float32)
        self.kint, self.vint = _codes(self.kq, kinds[0], D), _codes(self.vq, kinds[1], D)
        self.lo = view_lo(mode, T, window, kn is not None)
        self.kv_start = self.los = None
        if kv_start is not None:
            self.kv_start = clamp_starts(mode, kv_start, T, self.S)
            self.los = padded_los(mode, T, window, kn is not None, self.kv_start)

    def reference(self):
        """The oracle (the reference pipeline: dequantise to the compute dtype, cat the new token(s), softmax(q K^T) V).
        With ``kv_start`` the same pipeline with the per-row visibility of tests/attn_ref.py (the oracle has no start)."""
        d, c = self.dtype, self
        if c.kv_start is not None:
            from tests import attn_ref
            return attn_ref.of_case(c)
        if c.mode == "decode":
            return O.decode_attention(widen(c.q[:, :, 0], d), c.kq, c.ks, c.kinds[0], c.vq, c.vs, c.kinds[1], c.D, c.sm,
                                      None if c.kn is None else widen(c.kn, d), None if c.vn is None else widen(c.vn, d),
                                      kv_dtype=d, window=c.window)
        return O.extend_attention(widen(c.q, d), c.kq, c.ks, c.kinds[0], c.vq, c.vs, c.kinds[1], c.D, c.sm,
                                  widen(c.kn, d), widen(c.vn, d), kv_dtype=d, window=c.window)


def attend(c, drop=(), kswap=None, vswap=None, headmap="group", shift=0, drop_new=False, budget=None, wedge=0, wfirst=False,
           wchunk=True, past=0, dup_new=False, starts=None, wignore=False, drop_rows=None, past_rows=None,
           chunk_pad_seen=False, pad_row_v=False, dead_nonzero=False):
    """Float64 attention of case ``c`` with EXACT dequantised values (code x scale, what the kernels compute with), and
    optionally one deliberate mistake: ``drop`` stored tokens left out; ``kswap`` / ``vswap`` = t: the K / V scales of
    tokens t and t + 1 swapped; ``headmap="mod"``: query head h reads kv head h % Hkv instead of h // nq; ``shift``: the
    chunk mask moved by +-1 (row s sees chunk tokens j <= s + shift); ``drop_new``: the last chunk token (extend) / the new
    token (decode) left out. Returns [B,Hq,S,D] (extend) / [B,Hq,D] (decode).

    Under the case's window (the band is applied whenever ``c.window`` > 0): ``wedge`` = +1 / -1: every row's lower edge
    moved down / up by one (the row also sees p - W / misses p - W + 1); ``wfirst``: every row takes row 0's lower edge
    (extend without per-row edges); ``wchunk=False``: the chunk tokens' lower edge ignored (only the causal mask).

    Decode past a device-side count: ``past`` = n: n stored slots past the count attended as well, holding stale rows that
    a previous sequence over the same tokens could have left there: copies of the keys of the last n tokens, the new one
    included (cyclically when n is larger), with their values negated; ``dup_new``: the new token attended twice, the
    second time as its slot holds it once quantised (:func:`stored_new`).

    A left-padded case (``c.kv_start``): row b sees key k only from its start on, and a row that sees no key is zeros.
    ``starts``: [B] or [B, Hkv] starts used INSTEAD of the case's (an edge moved, another row's start, the start indexed
    by kv head); ``wignore``: batch rows with a start > 0 ignore the window; ``drop_rows`` = {b: stored tokens row b leaves
    out}; ``past_rows`` = {b: n}: ``past`` for row b alone; ``chunk_pad_seen`` (extend): rows at or past their start see
    the chunk tokens before it; ``pad_row_v`` (extend): a row whose own position is padding returns its own chunk token's
    V; ``dead_nonzero`` (decode without a new token): a row that sees no key attends every stored token instead.

    ``budget`` = (dtype, qplanes): also return the kernel-side error terms of :func:`bound` for this (unperturbed) case."""
    B, Hq, Hkv, T, D, S = c.B, c.Hq, c.Hkv, c.T, c.D, c.S
    pad = c.kv_start is not None
    nq = Hq // Hkv
    ks, vs = c.ks.astype(np.float64).copy(), c.vs.astype(np.float64).copy()
    if kswap is not None:
        ks[[kswap, kswap + 1]] = ks[[kswap + 1, kswap]]
    if vswap is not None:
        vs[[vswap, vswap + 1]] = vs[[vswap + 1, vswap]]
    K, V = c.kint * ks[:, None], c.vint * vs[:, None]
    svp = vs.copy()  # V scale in P' = e sv / svref (0: a token whose P is never rounded)
    if c.mode == "extend":
        new_k, new_v = widen(c.kn, c.dtype), widen(c.vn, c.dtype)
        svp = np.concatenate([svp, np.ones(S)])  # the chunk: tiles of scale 1 in the last split
    elif c.kn is not None:
        new_k, new_v = widen(c.kn, c.dtype)[:, :, None], widen(c.vn, c.dtype)[:, :, None]
        svp = np.concatenate([svp, [0.0]])  # decode's new token: folded in fp32 by the merge
    else:
        new_k = new_v = np.zeros((B, Hkv, 0, D))
    K, V = np.concatenate([K, new_k], axis=2), np.concatenate([V, new_v], axis=2)
    N, Nn = K.shape[2], new_k.shape[2]
    vis = np.ones((S, N), bool)
    for t in drop:
        vis[:, t] = False
    if Nn:
        j = np.arange(Nn)
        vis[:, T:] = j[None, :] <= np.arange(S)[:, None] + shift if c.mode == "extend" else True
        if drop_new:
            vis[:, N - 1] = False
    vis_nw = vis.copy() if pad else None  # before the window's band
    if c.window:
        pos = T + np.arange(S) if c.mode == "extend" else np.array([N - 1])  # the rows' positions
        edge = pos - c.window - wedge  # keys k <= edge are below the row's band
        if wfirst:
            edge = np.full_like(edge, edge[0])
        band = np.arange(N)[None, :] > edge[:, None]
        if not wchunk:
            band[:, T:] = True
        vis &= band
    if past_rows:
        past = max(past_rows.values())
    if past or dup_new:  # decode only: extra columns behind the new token, seen by the row
        idx = (N - past + np.arange(past)) % N
        sk, sv = stored_new(c) if dup_new else (None, None)
        xk = np.concatenate([K[:, :, idx]] + ([sk] if dup_new else []), axis=2)
        xv = np.concatenate([-V[:, :, idx]] + ([sv] if dup_new else []), axis=2)
        K, V = np.concatenate([K, xk], axis=2), np.concatenate([V, xv], axis=2)
        vis = np.concatenate([vis, np.ones((S, xk.shape[2]), bool)], axis=1)
        if pad:
            vis_nw = np.concatenate([vis_nw, np.ones((S, xk.shape[2]), bool)], axis=1)
        svp = np.concatenate([svp, np.zeros(xk.shape[2])])
    qf = widen(c.q, c.dtype)
    out = np.empty((B, Hq, S, D))
    terms = np.zeros((B, Hq, S, D))
    if budget:
        dtype, qplanes = budget
        svmax = svp[c.lo:].max() if svp[c.lo:].size else 0.0  # the view's scales only: the kernels never read [0, lo)
        ksum = np.abs(c.kint).sum(axis=-1) * c.ks.astype(np.float64)[None, None] * c.sm  # [B,Hkv,T]
    if pad:
        st_eff = np.asarray(c.kv_start if starts is None else starts, np.int64).reshape(B, -1)
        st_eff = np.broadcast_to(np.clip(st_eff, 0, T + S if c.mode == "extend" else T), (B, Hkv))
        kpos = np.arange(K.shape[2])
        qpos = T + np.arange(S) if c.mode == "extend" else np.array([N - 1])
    vis_all = vis
    for b in range(B):
        if pad:  # this batch row's own visibility
            vis0 = vis_nw.copy() if (wignore and c.kv_start[b] > 0) else vis_all.copy()
            if drop_rows and b in drop_rows:
                vis0[:, list(drop_rows[b])] = False
            if past_rows:  # the extra columns: the last past_rows[b] of them
                vis0[:, N + past - past_rows.get(b, 0):N + past] = True
                vis0[:, N:N + past - past_rows.get(b, 0)] = False
            if budget:  # this row's view [lo_b, T) plus the chunk: the kernels never read a scale before lo_b for row b
                svmax = svp[c.los[b]:].max() if svp[c.los[b]:].size else 0.0
        for h in range(Hq):
            g = h // nq if headmap == "group" else h % Hkv
            s = qf[b, h] @ K[b, g].T * c.sm
            if pad:
                seen = (kpos >= st_eff[b, g]) | (kpos >= N)
                if chunk_pad_seen:
                    seen = seen[None, :] | ((kpos >= T)[None, :] & (qpos >= st_eff[b, g])[:, None])
                vis = vis0 & seen
                if dead_nonzero:  # a row that sees no key attends every stored token instead
                    vis[~vis.any(axis=1)] = vis0[~vis.any(axis=1)]
                s[~vis] = -np.inf
                dead = ~vis.any(axis=1)
                p = np.exp(s - np.where(dead, 0.0, s.max(axis=1))[:, None])
                l = p.sum(axis=1, keepdims=True)
                l[dead] = 1.0
                out[b, h] = p / l @ V[b, g]
                if pad_row_v:
                    out[b, h][dead] = V[b, g][T:N][dead]
                if not budget:
                    continue
            else:
                s[~vis] = -np.inf
                p = np.exp(s - s.max(axis=1, keepdims=True))
                l = p.sum(axis=1, keepdims=True)
                out[b, h] = p / l @ V[b, g]
                if not budget:
                    continue
            # P' rounding: relative P_REL where e sv / svmax is normal, absolute P_ABS below it (in units of svref <= svmax)
            rnd = svp[None, :] > 0
            normal = p * svp[None, :] >= P_MIN[dtype] * svmax
            a = np.where(rnd & normal, P_REL[dtype] * p, 0.0)
            a += np.where(rnd & ~normal & vis, P_ABS[dtype] * svmax / np.where(svp > 0, svp, 1.0)[None, :], 0.0)
            terms[b, h] += a / l @ np.abs(V[b, g])
            if qplanes and c.kinds[0] == "int8" and T:
                delta = (ksum[b, g] * np.abs(qf[b, h]).max(axis=-1)[:, None] * QPLANE * vis[:, :T]).max(axis=1)  # [S]
                w = p / l
                spread = np.einsum("sn,snd->sd", w, np.abs(V[b, g][None] - out[b, h][:, None]))
                terms[b, h] += np.expm1(2.0 * delta)[:, None] * spread
    if c.mode == "decode":
        out, terms = out[:, :, 0], terms[:, :, 0]
    return (out, terms) if budget else out


def stored_new(c):
    """decode's new token as its store slot holds it after the step: the oracle's codes x scale, K and V [B,Hkv,1,D]"""
    odt = "bf16" if c.dtype == "bf16" else None
    out = []
    for x, kind in ((c.kn, c.kinds[0]), (c.vn, c.kinds[1])):
        q, _, s = O.quantize_tokens(x[None, :, :, None, :], kind, dtype=odt)
        out.append(_codes(q[0], kind, c.D) * s[0].astype(np.float64)[None, None, :, None])
    return out


def bound(c, ref, qplanes=False):
    """Per-element error budget of a kernel result against the oracle ``ref`` (float64, same shape):

        TOL[dtype] * (|ref| + max_d |ref|)                   the suite's standard tolerance (output rounding + slack),
                                                             scaled by each output row's own largest element instead
                                                             of the whole tensor's (a sink row's output is 100x smaller
                                                             than a probe row's: the tensor-wide form would hide it)
      + |ref - exact|                                        the oracle rounds the dequantised K / V to the compute dtype,
                                                             the kernels multiply the exact codes by the scales: computed
                                                             exactly, the float64 attention over code x scale (`attend`)
      + sum_t c_t |v_t| / l                                  P' = e_t sv_t / svref rounded to f16 / bf16 before P V, with
                                                             e_t = exp(s_t - m) <= 1 against the running max, svref <=
                                                             svmax (largest V scale the walk can see; the chunk's tiles
                                                             have scale 1): c_t = P_REL e_t where e_t sv_t / svmax is a
                                                             normal number (relative 2^-11 f16, 2^-8 bf16), else
                                                             c_t = 2^-25 svmax / sv_t (an absolute 2^-25 on P' in units
                                                             of svref). Later rescales multiply P' and its error alike.
      + expm1(2 Delta) sum_t p_t |v_t - out|                 INT8 keys in the decode MFMA kernels: the query as two int8
                                                             planes, error <= max|q| / 64,516 per element, so every score
                                                             moves by at most Delta = max_t sm sk_t sum_d |k_int| max|q|
                                                             / 64,516; softmax weights then move by a factor within
                                                             exp(+-2 Delta) and the output by at most this.

    A left-padded case (``c.kv_start``): every visibility is the batch row's own (its start and the band), svmax is taken
    per batch row from that row's view [lo_b, T) plus the chunk, and a row that sees no key has budget 0: :func:`check`
    compares it with == 0.

    Under a window (``c.window`` > 0) every visibility above is the band's (row s sees p - W < k <= p), and svmax is the
    largest V scale of the VIEW, stored tokens [lo, T) (decode's lo, extend's lo0) plus the chunk's 1: the kernels start
    the store at lo (host count) or add lo to their row base (device count), so no scale before lo, nor past the count,
    can enter the running V-scale max.

    The terms are computed from the case's own data (scores, weights, values, scales), never a larger constant."""
    exact, terms = attend(c, budget=(c.dtype, qplanes))
    return TOL[c.dtype] * (np.abs(ref) + np.abs(ref).max(axis=-1, keepdims=True)) + np.abs(ref - exact) + terms


def check(got, ref, bud):
    """(passes, worst err / budget). A non-finite result fails."""
    got = np.asarray(got, np.float64)
    if not np.isfinite(got).all():
        return False, float("inf")
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):  # budget 0 (a left-padded row that sees no key): exact or rejected
        r = float(np.where(bud > 0, err / bud, np.where(err == 0, 0.0, np.inf)).max())
    return r <= 1.0, r


# ------------------------------------------------------------------------------------------------------------ builders

def _positions(T, splits):
    """Stored probe targets: 0, 63, 64, T - 1 and both sides of every split boundary (splits = tokens per split)."""
    pos = {0, 63, 64, T - 1}
    for sp in splits:
        firsts = list(range(sp, T, sp))
        for k in firsts[:3] + firsts[-2:]:
            pos |= {k - 1, k}
    return sorted(p for p in pos if 0 <= p < T)


def _edge_rows(T, S, W, lo, splits):
    """Extend rows whose lower edges get probes: the first and last rows, rows around s = W (the edge enters the chunk)
    and rows whose edge p - W + 1 = T + s + 1 - W falls next to a 64-token tile or split boundary of the view."""
    rows = {0, 1, 2, S - 2, S - 1, W - 2, W - 1, W, W + 1}
    for b in [64, 128] + [sp * k for sp in splits for k in (1, 2)]:
        for d in (-1, 0, 1):
            rows.add(lo + b + d - (T + 1 - W))
    return sorted(r for r in rows if 0 <= r < S)


def make_case(family, mode, B, Hq, Hkv, T, S, D, kinds, dtype, seed=0, splits=(), with_new=True, variant=None,
              factor=16.0, probe_every=2, window=0, targets=None, kv_start=None):
    """Build a case (see the module docstring). ``splits``: tokens per split of the routes the case will run on (their
    boundaries get probes; under a window, counted from the view's first token). ``probe_every``: 1 / probe_every of the
    query rows, picked at random, are probes (family ``probe``: all). ``window``: see the module docstring. ``targets``
    (decode): the stored probe targets instead, in the order the probe rows take them, after the new token.
    ``kv_start``: B key starts, a left-padded batch (:func:`_make_padded_case`; None changes nothing)."""
    if kv_start is not None:
        assert targets is None and factor == 16.0, "a padded case chooses its own targets; no outlier family"
        return _make_padded_case(family, mode, B, Hq, Hkv, T, S, D, kinds, dtype, seed, splits, with_new, variant, window,
                                 kv_start, probe_every)
    rng = np.random.default_rng(seed)
    W = window
    lo = view_lo(mode, T, W, with_new)
    nq = Hq // Hkv
    Sq = S if mode == "extend" else 1
    H = hadamard(D)
    sq = np.sqrt(D)
    sm = 1.0 / sq
    Sn = S if mode == "extend" else (1 if with_new else 0)
    # background: small keys and values (the probes' targets dominate their tokens' scales), queries per family
    sig_k = 1.0 if family == "outlier" else 0.1
    k = rng.standard_normal((B, Hkv, T + Sn, D)) * sig_k
    v = rng.standard_normal((B, Hkv, T + Sn, D)) * 0.5
    q = rng.standard_normal((B, Hq, Sq, D)) * 0.5
    if family == "outlier":
        ch = [3, D // 2 + 5]
        k[..., ch] *= factor
        q[..., ch] *= factor
    nv = T - lo  # the view [lo, T) (no window: the whole store)
    if family == "vrange":  # per-token V scales over four decades: large first, the attended (smallest) ones last
        u = rng.uniform(-4.0, 0.0, T + Sn)
        u[lo: lo + nv // 2] = rng.uniform(-1.0, 0.0, nv // 2)
        u[T - nv // 4: T] = rng.uniform(-4.0, -3.5, nv // 4)
        v *= 10.0 ** u[None, None, :, None]
    # rows (b, h, s): a random 1 / probe_every of them are probes (family "probe": all), chunk row S - 1 always
    rows = [(b, h, s) for b in range(B) for h in range(Hq) for s in range(Sq)]
    every = 1 if family == "probe" else probe_every
    pick = rng.permutation(len(rows))[: max(1, len(rows) // every)]
    probe_rows = [rows[i] for i in sorted(pick)]
    if mode == "extend" and (0, 0, Sq - 1) not in probe_rows:
        probe_rows.append((0, 0, Sq - 1))
    # window: rows that aim at their own lower edge, "in" (p - W + 1, seen) or "out" (p - W, must stay unseen)
    edge_of = {}
    if W:
        if mode == "extend":
            for s_ in _edge_rows(T, S, W, lo, splits):
                for h_, e in ((s_ % Hq, "in"), ((s_ + 1) % Hq, "out")):
                    if (0, h_, s_) != (0, 0, Sq - 1):  # that row keeps its chunk probe
                        edge_of[(0, h_, s_)] = e
        else:
            for i, r in enumerate(probe_rows[:2]):
                edge_of[r] = ("in", "out")[i % 2]
        # the edge rows and the last chunk row first: they must not run out of probe directions
        first = [r for r in sorted(set(edge_of) | {(0, 0, Sq - 1)}) if r in edge_of or mode == "extend"]
        probe_rows = first + sorted((set(probe_rows) | set(edge_of)) - set(first))
    fam_rows = sorted(set(rows) - set(probe_rows))
    fam_dir = H[1]
    if family == "outlier":  # the outlier channels are `factor` x the query's own rms
        for b, h, s in fam_rows:
            q[b, h, s] /= factor
    if family in ("sink", "vrange", "late"):
        for b, h, s in fam_rows:
            q[b, h, s] = rng.standard_normal(D) * 0.05
    t_sink = None
    if family == "sink":
        # variant "lo": decode's first visible token; extend's last row's first visible one (every row sees it)
        t_lo = min(lo + (Sq - 1 if mode == "extend" else 0), T - 1)
        t_sink = T if (variant == "chunk" or T == 0) else (t_lo if variant == "lo" else 0)
        a_s = 2.0
        k[:, :, t_sink] += a_s * fam_dir
        v[:, :, t_sink] *= 0.01
        for b, h, s in fam_rows:
            q[b, h, s] += rng.uniform(12.0, 20.0) / (a_s * sq) * fam_dir
    elif family == "vrange":
        focus = np.arange(T - nv // 4, T)
        k[:, :, focus] += 1.5 * fam_dir
        for b, h, s in fam_rows:
            q[b, h, s] += 10.0 / (1.5 * sq) * fam_dir
    elif family == "late":
        z = rng.uniform(-150.0, 0.0, T + Sn)
        if W and T > lo:  # the window's lower edge
            top = np.arange(lo, min(lo + 64, T))
        else:
            top = np.arange(max(0, T - 64), T) if (mode == "decode" and T) else np.arange(T, T + Sn)
        hot = rng.choice(top, size=min(4, len(top)), replace=False)
        z[hot] = rng.uniform(140.0, 150.0, len(hot))
        z[hot[0]] = 150.0
        k += (z / sq)[None, None, :, None] * fam_dir
        for b, h, s in fam_rows:
            q[b, h, s] += fam_dir
    # probes: each row gets a target token; one Hadamard direction per target within its (batch row, kv head)
    stored = [lo + t for t in _positions(T - lo, splits) if lo + t != t_sink]
    if targets is not None:
        stored = [t for t in dict.fromkeys(targets) if 0 <= t < T and t != t_sink]
    kinds_ = [("t", t) for t in stored] + ([("n", 0)] if mode == "decode" and Sn else [])
    if W or targets is not None:  # decode: the new token first, so that a few rows cover it too
        kinds_ = kinds_[-1:] + kinds_[:-1] if mode == "decode" and Sn else kinds_
    dirs, used, kamp = {}, {}, {}
    # a target's key amplitude dominates its token's scale (over the family's own key components), so that a swapped
    # scale moves the probe
    base = {"outlier": 6.0 * factor, "vrange": 4.0, "late": 30.0}.get(family, 1.0)
    n_ext = n_st = 0
    last_row = False  # a probe on chunk token S - 1 exists
    for i, (b, h, s) in enumerate(probe_rows):
        g = h // nq
        p = T + s if mode == "extend" else (T if Sn else T - 1)  # the row's position
        vis_lo = p + 1 - W if W else 0  # the first key it sees
        edge = edge_of.get((b, h, s))
        is_edge = bool(edge) and p - W + (edge == "in") >= 0 and p - W + (edge == "in") != t_sink
        if is_edge:
            tok = p - W + (edge == "in")
        elif W and mode == "extend" and (s == Sq - 1 and not last_row or i % 3 == 2 or
                                         not any(t >= vis_lo for _, t in kinds_)):
            last_row |= s == Sq - 1
            n_ext += s < Sq - 1
            tok = T + s + 1 if (n_ext % 2 == 0 and s < Sq - 1) else T + s
        elif W and mode == "extend":  # the next stored target the row sees
            while kinds_[n_st % len(kinds_)][1] < vis_lo:
                n_st += 1
            tok = kinds_[n_st % len(kinds_)][1]
            n_st += 1
        elif mode == "extend" and ((s == Sq - 1 and not last_row) or i % 3 == 2 or not kinds_):
            last_row |= s == Sq - 1
            # chunk targets: the diagonal j = s, or (every other one) the future token j = s + 1, which must stay unseen
            n_ext += s < Sq - 1
            tok = T + s + 1 if (n_ext % 2 == 0 and s < Sq - 1) else T + s
        else:
            kind, idx = kinds_[n_st % len(kinds_)]
            n_st += 1
            tok = idx if kind == "t" else T
        key = (b, g, tok)
        if key not in dirs:
            if used.get((b, g), 0) >= D - 2:
                # out of probe directions: a window-edge row must never be the one left without its target
                assert not is_edge, ("window edge probe without a direction", (b, h, s), edge, D)
                continue
            dirs[key] = H[2 + used.get((b, g), 0)]
            used[(b, g)] = used.get((b, g), 0) + 1
            kamp[key] = base * (1.0 + 2.0 * (tok % 2))  # adjacent targets: x1 / x3
            k[b, g, tok] += kamp[key] * dirs[key]
            v[b, g, tok] = rng.standard_normal(D) * (2.0 if tok % 2 == 0 else 6.0)
        qrow = 18.0 / (kamp[key] * sq) * dirs[key]
        if family == "outlier":
            qrow[ch] = 0.0
        q[b, h, s] = qrow
    k_all, v_all, q = narrow(k, dtype), narrow(v, dtype), narrow(q, dtype)
    k_st, v_st = k_all[:, :, :T], v_all[:, :, :T]
    if mode == "extend":
        kn, vn = k_all[:, :, T:], v_all[:, :, T:]
    elif Sn:
        kn, vn = np.ascontiguousarray(k_all[:, :, T]), np.ascontiguousarray(v_all[:, :, T])
    else:
        kn = vn = None
    info = dict(family=family, variant=variant, factor=factor, stored=stored, splits=tuple(splits), window=W)
    return Case(mode, dtype, kinds, sm, q, np.ascontiguousarray(k_st), np.ascontiguousarray(v_st),
                None if kn is None else np.ascontiguousarray(kn), None if vn is None else np.ascontiguousarray(vn), info,
                window=W)


def _make_padded_case(family, mode, B, Hq, Hkv, T, S, D, kinds, dtype, seed, splits, with_new, variant, W, kv_start,
                      probe_every):
    """A left-padded case: row b of the batch sees key k only from ``kv_start[b]`` on, so every probe target,
    every family's hot spot and every edge is placed per batch row, from the row's own first visible key.

    ``splits``: tokens per split, counted from each row's own lo_b: one tuple for every row, or B tuples (the ring spreads
    row b's live tiles by its own count). Decode: row b's probe rows aim, in this order, at its first visible key ("in":
    lo_b, or the new token when lo_b = T), at the key before it ("out", 18 nats and a V of its own like the window's
    forbidden target: padding for row b, or a real token below the window's bound, in a slot whose scale the row with
    start 0 needs, so no store can leave it out), the new token, T - 1, both sides of the row's last live split's first
    token, then lo_b + _positions(T - lo_b, splits_b). The "in" and "out" probes of row b sit on heads of kv heads b + 1
    and b + 2 (mod Hkv), so that a start indexed by kv head moves them. Extend: "in" / "out" probes on rows s0 = start_b -
    T (the first row whose own position is not padding), s0 + 1, S - 1 and, under a window, around the row where the
    window's bound overtakes the start; the other rows take stored targets they see, their diagonal token and the future
    one in turn. Rows that see no key keep a Gaussian query: their output is zero. ``info["start_probes"]`` counts each
    batch row's edge probes."""
    assert family in ("probe", "sink", "late", "vrange") and len(kv_start) == B, (family, kv_start, B)
    rng = np.random.default_rng(seed)
    ext = mode == "extend"
    Sq = S if ext else 1
    Sn = S if ext else (1 if with_new else 0)
    N = T + Sn
    st = clamp_starts(mode, kv_start, T, S)
    assert min(st) == 0, ("one row must start at 0: it needs every slot's scale", st)
    lo0 = view_lo(mode, T, W, with_new)
    los = padded_los(mode, T, W, with_new, st)
    rows_splits = [tuple(x) for x in splits] if (splits and isinstance(splits[0], (tuple, list))) else [tuple(splits)] * B
    nq = Hq // Hkv
    H = hadamard(D)
    sq = np.sqrt(D)
    pos = [T + s for s in range(Sq)] if ext else [T if Sn else T - 1]  # the rows' positions

    def first(b, s):  # the first key row (b, s) sees; the row sees none when it is past its position
        return max(st[b], pos[s] + 1 - W if W else 0)

    k = rng.standard_normal((B, Hkv, N, D)) * 0.1
    v = rng.standard_normal((B, Hkv, N, D)) * 0.5
    q = rng.standard_normal((B, Hq, Sq, D)) * 0.5
    fam_dir = H[1]
    sinks = [None] * B
    if family == "sink" and N:
        for b in range(B):
            if variant == "lo":  # the row's own first visible key (extend under a window: the last row's)
                sinks[b] = min(max(st[b], lo0 + (Sq - 1 if (ext and W) else 0)), N - 1)
            else:
                sinks[b] = 0  # rows with a start > 0 must not see it
    sink_slots = {t for t in sinks if t is not None}
    # ---- probe rows and their targets: (b, h, s, token, "in" / "out" / None), edge probes first
    assign, taken = [], set()
    for b in range(B):
        if ext:
            s0 = max(0, st[b] - T)
            if s0 >= Sq:
                continue
            edge_rows = {s0, s0 + 1, Sq - 1}
            if W:
                sx = st[b] + W - 1 - T  # the row at which the window's bound reaches the start
                edge_rows |= {sx - 1, sx, sx + 1, W - 1, W}
            for s in sorted(r for r in edge_rows if s0 <= r < Sq):
                f = first(b, s)
                for h, e, tok in (((s + b) % Hq, "in", f), ((s + b + 1) % Hq, "out", f - 1)):
                    if tok >= 0 and (b, h, s) not in taken and Hq > 1:
                        assign.append((b, h, s, tok, e))
                        taken.add((b, h, s))
            stored = [lo0 + t for t in _positions(T - lo0, rows_splits[b]) if lo0 + t >= los[b]]
            stored += [los[b] + t for t in _positions(T - los[b], ())]
            stored = [t for t in dict.fromkeys(stored) if t not in sink_slots]
            rest = [(b, h, s) for s in range(s0, Sq) for h in range(Hq) if (b, h, s) not in taken]
            every = 1 if family == "probe" else probe_every
            pick = sorted(rng.permutation(len(rest))[: max(1, len(rest) // every)]) if rest else []
            n_st = n_ext = 0
            for i, j in enumerate(pick):
                _, h, s = rest[j]
                seen = [t for t in stored if t >= first(b, s)]
                if i % 3 == 2 or not seen:  # the diagonal token, or (every other one) the future token it must not see
                    n_ext += s < Sq - 1
                    tok = T + s + 1 if (n_ext % 2 == 0 and s < Sq - 1) else T + s
                else:
                    tok = seen[n_st % len(seen)]
                    n_st += 1
                assign.append((b, h, s, tok, None))
        else:
            f = first(b, 0)
            if f > pos[0]:
                continue  # the row sees no key
            heads = sorted(range(Hq), key=lambda h: (h % nq, (h // nq - b - 1) % Hkv))
            n_probe = Hq if family == "probe" else max(min(Hq, 3), Hq // max(1, probe_every))
            order = [(f, "in")] + ([(f - 1, "out")] if f >= 1 else [])
            more = ([T] if Sn else []) + [T - 1]
            lt = T - los[b]
            for sp in rows_splits[b]:
                if lt > sp:
                    last = los[b] + (lt - 1) // sp * sp
                    more += [last - 1, last]
            more += [los[b] + t for t in _positions(lt, rows_splits[b])]
            got = {t for t, _ in order}
            for t in more:
                if f <= t < N and t not in got and t not in sink_slots:
                    order.append((t, None))
                    got.add(t)
            for i, h in enumerate(heads[:n_probe]):
                tok, e = order[i % len(order)]
                assign.append((b, h, 0, tok, e))
                taken.add((b, h, 0))
    # ---- the family's tokens. One scale per slot is shared by every batch row and head, so a slot that holds a probe
    # target (a large K and V in one (row, kv head)) quantises every other row's token there to codes near 0. A token
    # that carries a family row's weight must not sit in such a slot: its V would be 0 x a large scale, the row's output
    # 1e-5 of that scale, and the fp32 rounding of the kernels' biased V sum (2^-24 x bias x sum p sv, which the budget
    # does not model) would be of the output's size. So the hot tokens and the attended V range avoid target slots, and
    # a sink's slot holds a small V in EVERY row (the slot's scale stays small; a probe aimed at it returns that V).
    tslots = {tok for _, _, _, tok, _ in assign}
    if family == "vrange":  # one V scale per slot, shared by the rows: the largest at the bottom of EVERY row's view
        u = rng.uniform(-4.0, 0.0, N)
        nvs = sorted({T - l for l in los if l < T}, reverse=True)
        for nv in nvs:
            u[T - nv: T - nv + nv // 2] = rng.uniform(-1.0, 0.0, nv // 2)
        nf = max(1, nvs[-1] // 4) if nvs else 0  # the attended smallest: the top quarter of the shortest view
        u[T - nf: T] = rng.uniform(-4.0, -3.5, nf)
        v *= 10.0 ** u[None, None, :, None]
        focus = np.array([t for t in range(T - nf, T) if t not in tslots], np.int64)
        k[:, :, focus] += 1.5 * fam_dir
    elif family == "sink" and N:
        for b in range(B):
            k[b, :, sinks[b]] += 2.0 * fam_dir
        for t in sink_slots:
            v[:, :, t] *= 0.01
    elif family == "late" and N:
        z0 = rng.uniform(-150.0, 0.0, N)
        for b in range(B):  # the hot tokens: in each row's first 64 visible tokens
            z = z0.copy()
            f = min(max(st[b], lo0), N - 1)
            top = np.arange(f, min(f + 64, T if f < T else N))
            free = np.array([t for t in top if t not in tslots], np.int64)
            top = free if len(free) else top
            hot = rng.choice(top, size=min(4, len(top)), replace=False)
            z[hot] = rng.uniform(140.0, 150.0, len(hot))
            z[hot[0]] = 150.0
            k[b] += (z / sq)[None, :, None] * fam_dir
    taken = {(b, h, s) for b, h, s, _, _ in assign}
    live_rows = [(b, h, s) for b in range(B) for h in range(Hq) for s in range(Sq) if first(b, s) <= pos[s]]
    fam_rows = [r for r in live_rows if r not in taken]
    if family in ("sink", "vrange", "late"):
        for b, h, s in fam_rows:
            q[b, h, s] = rng.standard_normal(D) * 0.05
            if family == "sink":
                q[b, h, s] += rng.uniform(12.0, 20.0) / (2.0 * sq) * fam_dir
            elif family == "vrange":
                q[b, h, s] += 10.0 / (1.5 * sq) * fam_dir
            else:
                q[b, h, s] += fam_dir
    dirs, used, kamp = {}, {}, {}
    base = {"vrange": 4.0, "late": 30.0}.get(family, 1.0)
    n_edge = {b: {"in": 0, "out": 0} for b in range(B)}
    for b, h, s, tok, e in assign:
        g = h // nq
        key = (b, g, tok)
        if key not in dirs:
            if used.get((b, g), 0) >= D - 2:
                # out of probe directions: a start-edge (or window-edge) probe must never be the one left out
                assert e is None, ("edge probe without a direction", (b, h, s), e, D)
                continue
            dirs[key] = H[2 + used.get((b, g), 0)]
            used[(b, g)] = used.get((b, g), 0) + 1
            kamp[key] = base * (1.0 + 2.0 * (tok % 2))
            k[b, g, tok] += kamp[key] * dirs[key]
            if tok not in sink_slots:  # an edge probe on a sink's slot keeps the small V: the probe row returns that
                v[b, g, tok] = rng.standard_normal(D) * (2.0 if tok % 2 == 0 else 6.0)
        q[b, h, s] = 18.0 / (kamp[key] * sq) * dirs[key]
        if e:
            n_edge[b][e] += 1
    k_all, v_all, q = narrow(k, dtype), narrow(v, dtype), narrow(q, dtype)
    kn = vn = None
    if ext:
        kn, vn = np.ascontiguousarray(k_all[:, :, T:]), np.ascontiguousarray(v_all[:, :, T:])
    elif Sn:
        kn, vn = np.ascontiguousarray(k_all[:, :, T]), np.ascontiguousarray(v_all[:, :, T])
    info = dict(family=family, variant=variant, factor=16.0, stored=None, splits=tuple(rows_splits), window=W,
                start_probes=n_edge, sinks=sinks)
    return Case(mode, dtype, kinds, 1.0 / sq, q, np.ascontiguousarray(k_all[:, :, :T]), np.ascontiguousarray(v_all[:, :, :T]),
                kn, vn, info, window=W, kv_start=st)


def padded_live(plan, lt):
    """(tokens per live split, live split count) of a batch row with ``lt`` visible stored tokens in a padded launch
    planned as ``plan`` (:func:`dev_plan` for the count, or for what the window leaves of it): padded_split_tokens in
    csrc/attn/common.inc. The ring spreads the row's own ceil(lt / 64) tiles over the launch's nsplit waves; every other
    route keeps the host's split size. Splits are counted from the row's lo_b."""
    ts = plan.ts
    if plan.tpw:
        ts = max(1, -(-(-(-lt // STREAM_TC)) // plan.nsplit)) * STREAM_TC
    return ts, -(-lt // ts)


def padded_plan(B, Hq, Hkv, D, k_bits, T, W=0, with_new=True, tunables=None, v_bits=4):
    """The plan of a padded decode call over T stored tokens (host count, or the bound of a device count): planned for
    what the window alone leaves visible, min(T, W - 1) stored tokens beside a new token, min(T, W) without one."""
    return dev_plan(B, Hq, Hkv, D, k_bits, min(T, W - (1 if with_new else 0)) if W else T, tunables, v_bits=v_bits)


def padded_first(c, starts=None, wignore=False):
    """[B, Hkv, S] (decode: S = 1): the first key each (batch row, kv head, query row) of the left-padded case ``c`` sees,
    its position + 1 where it sees none; with ``starts`` ([B] or [B, Hkv]) used instead of the case's and ``wignore``
    as :func:`attend` takes them."""
    B, Hkv, T, S = c.B, c.Hkv, c.T, c.S
    ext = c.mode == "extend"
    qpos = T + np.arange(S) if ext else np.array([T - (c.kn is None)])  # the rows' positions
    wlo = qpos + 1 - c.window if c.window else np.zeros_like(qpos)
    eff = np.asarray(c.kv_start if starts is None else starts, np.int64)
    eff = np.broadcast_to(np.reshape(np.clip(eff, 0, T + S if ext else T), (B, -1)), (B, Hkv))
    wlo = np.broadcast_to(wlo[None, None, :], (B, Hkv, len(qpos))).copy()
    if wignore:
        wlo[np.asarray(c.kv_start) > 0] = 0
    return np.minimum(np.maximum(eff[:, :, None], wlo), qpos[None, None, :] + 1)


def padded_perturbations(c, plan=None):
    """Every deliberate mistake of a left-padded launch that changes what some row of case ``c`` sees: (name, kwargs of
    :func:`attend`). ``plan`` (decode): the launch's :func:`padded_plan`, for the mistakes in a row's live split count."""
    B, Hkv, T, S = c.B, c.Hkv, c.T, c.S
    ext = c.mode == "extend"
    st = np.asarray(c.kv_start, np.int64)
    hi = T + S if ext else T
    out = []

    def add(name, eff):  # only where some row then sees other keys (under a window the start may never win)
        if not np.array_equal(padded_first(c, eff), padded_first(c)):
            out.append((name, dict(starts=np.asarray(eff))))
    add("start edge +1", np.clip(st + 1, 0, hi))
    add("start edge -1", np.clip(st - 1, 0, hi))
    add("row 0's start for every row", np.full(B, st[0]))
    add("row (b + 1) % B's start for row b", np.roll(st, -1))
    if B > 1 and Hkv > 1:
        add("start indexed by kv head", np.repeat(st[np.arange(Hkv) % B][None, :], B, axis=0))
    if c.window:
        p_last = T + S - 1 if ext else T - (c.kn is None)  # the last row's position
        if (st > c.lo).any():
            add("start ignored under the window", np.zeros(B, np.int64))
        if ((st > 0) & (st < p_last + 1 - c.window)).any():
            out.append(("window ignored where a start is set", dict(wignore=True)))
    if plan is not None and not ext:
        ts_u = plan.live(T)[0]
        d_u, d_last, dead = {}, {}, {}
        for b in range(B):
            lt = T - c.los[b]
            ts, ns = padded_live(plan, lt)
            ns_u = -(-lt // ts_u)
            if ns_u < ns:
                d_u[b] = range(c.los[b] + ns_u * ts, T)
            if ns > 1:
                d_last[b] = range(c.los[b] + (ns - 1) * ts, T)
            if ns < plan.nsplit and (T or c.kn is not None):
                dead[b] = ts
        if d_u:
            out.append((f"live splits counted with the unpadded split size {ts_u} (rows {sorted(d_u)})", dict(drop_rows=d_u)))
        if d_last:
            out.append((f"last live split dropped (rows {sorted(d_last)})", dict(drop_rows=d_last)))
        if dead:
            out.append((f"first dead split attended (rows {sorted(dead)})", dict(past_rows=dead)))
    if ext:
        if ((st > T) & (st < T + S)).any():
            out.append(("chunk tokens before the start seen by later rows", dict(chunk_pad_seen=True)))
        if (st > T).any():
            out.append(("padding rows given their own token's V", dict(pad_row_v=True)))
    elif c.kn is None and (st >= T).any():
        out.append(("a row that sees no key is not zero", dict(dead_nonzero=True)))
    return out


def perturbations(c):
    """Every deliberate mistake that applies to case ``c``: (name, kwargs of :func:`attend`)."""
    T, lo = c.T, c.lo  # positions relative to the view's start (no window: lo = 0)
    out = []
    firsts = sorted({lo + k for sp in c.info["splits"] for k in range(sp, T - lo, sp)})
    for t in sorted({lo, lo + 63, lo + 64, T - 1} | set(firsts[:3])):
        if lo <= t < T:
            out.append((f"drop stored {t}", dict(drop=(t,))))
    for t in sorted({lo, lo + 63, T - 2} | set(f - 1 for f in firsts[:2])):
        if lo <= t < T - 1:
            out.append((f"K scales {t}<->{t + 1}", dict(kswap=t)))
            out.append((f"V scales {t}<->{t + 1}", dict(vswap=t)))
    if c.Hkv > 1 and c.Hq // c.Hkv > 1:
        out.append(("head map h % Hkv", dict(headmap="mod")))
    if c.mode == "extend":
        if c.S > 1:
            out.append(("chunk mask +1", dict(shift=1)))
        out.append(("chunk mask -1", dict(shift=-1)))
        out.append(("last chunk token dropped", dict(drop_new=True)))
    elif c.kn is not None:
        out.append(("new token left out", dict(drop_new=True)))
    if c.window:
        W = c.window
        p_last = T + c.S - 1 if c.mode == "extend" else T - (c.kn is None)  # the last row's position
        if p_last - W >= 0:
            out.append(("window edge +1", dict(wedge=1)))
        if p_last - W + 1 >= 0:
            out.append(("window edge -1", dict(wedge=-1)))
        if c.mode == "extend" and c.S > 1 and p_last - W >= 0:
            out.append(("first row's edge for every row", dict(wfirst=True)))
        if c.mode == "extend" and c.S > W:
            out.append(("chunk lower edge ignored", dict(wchunk=False)))
    return out


def dev_perturbations(c, p, count):
    """The mistakes of a device-count decode step (plan ``p`` from :func:`dev_plan`) on case ``c`` at device count
    ``count`` (c.T = the count clamped to the bound): the merge's live splits counted with the host's split size (the
    bound's) instead of the count's; the last live split dropped; the first dead split's slots attended; at count 0
    stored slot 0 attended; the new token attended twice, once from its slot (from count 2 on, with INT4 values: at count
    0 the output is the new token's V whatever its weight; at count 1, or with INT8 values, the slot's copy of the new
    token can sit within the rounding budget of the exact one for the rows that aim at it)."""
    t = c.T
    ts, ns = p.live(count)
    out = []
    ns_host = -(-t // p.ts)
    if ns_host < ns:
        out.append((f"split size {p.ts} from the bound", dict(drop=tuple(range(ns_host * ts, t)))))
    if ns > 1:
        out.append((f"last live split dropped (split {ns - 1})", dict(drop=tuple(range((ns - 1) * ts, t)))))
    if ns < p.nsplit:
        out.append((f"first dead split attended ({ts} slots)", dict(past=ts)))
    if t == 0:
        out.append(("stored slot 0 attended at count 0", dict(past=1)))
    elif t > 1 and c.kinds[1] == "int4":
        out.append(("new token attended twice", dict(dup_new=True)))
    return out
