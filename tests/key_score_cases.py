"""The float64 model of ``kvq_key_scores`` (include/kvq_hip.h) and the inputs its tests run on (numpy, CPU), shared by
tests/test_key_score_model.py (CPU: the model is right and the check rejects wrong answers) and tests/test_gpu_key_scores.py
(GPU: the kernels pass it).

The ``S`` query rows are the queries of the LAST ``S`` stored tokens: row ``s`` sits at position ``T - S + s`` and sees the
stored keys ``t <= T - S + s``. With ``nq = Hq / Hkv`` and ``hk = h // nq``::

    sc[h, s, t]     = sm_scale * k_scales[t] * sum_d q[b, h, s, d] * k_int[b, hk, t, d]
    p[h, s, :]      = softmax of sc over the visible t
    mass[b, hk, t]  = sum over the nq heads of hk, over the rows s that see t, of p[h, s, t]

on the exact code x scale values (no rounding of the dequantised key). A case is one layer's inputs, built from a seed and
quantised by ``oracle.kvq_oracle.quantize_tokens``:

* ``flat``: Gaussian q and k (soft distributions: every key matters to every row);
* ``probe``: every query row carries a Hadamard direction that one target key of its kv head carries, about 18 nats above
  the rest, so that the target's mass is the number of rows pointing at it. Targets: 0, 63, 64, T - S - 1, T - S, T - 1,
  each row's own position, and the position one past a row, which must receive nothing from that row;
* ``scale_span``: ``k_scales`` log-uniform over four decades.

:func:`key_mass` also takes one deliberate mistake, for the discrimination test."""
import numpy as np

from oracle import kvq_oracle as O
from tests.attn_cases import TOL, _codes, hadamard, narrow, widen

QB, TC, MAX_SPLIT, TARGET_WG = 64, 64, 64, 1024
FAMILIES = ("flat", "probe", "scale_span")


def plan(B, Hq, Hkv, T, S):
    """Python restatement of the launch plan (csrc/kvq_scores.hip): (query blocks, pass-1 splits, tiles per split,
    pass-2 runs, tiles per run)."""
    M = S * (Hq // Hkv)
    nqb = -(-M // QB)
    ntiles = -(-T // TC)
    base = nqb * B * Hkv
    ns = max(1, min(-(-TARGET_WG // base), (ntiles + 1) // 2, MAX_SPLIT))
    per = -(-ntiles // ns)
    nruns = min(ntiles, -(-TARGET_WG // (B * Hkv)))
    tpr = -(-ntiles // nruns)
    return nqb, -(-ntiles // per), per, -(-ntiles // tpr), tpr


def kernel_names(B, Hq, Hkv, T, S, D, kind, dtype):
    """What the kernel log shows for one call: pass 1, the split merge when pass 1 is split, pass 2."""
    targs = f"<{8 if kind == 'int8' else 4}, {D}, {1 if dtype == 'bf16' else 0}>"
    merge = ["key_scores_lse_k"] if plan(B, Hq, Hkv, T, S)[1] > 1 else []
    return ["key_scores_stats_k" + targs] + merge + ["key_scores_mass_k" + targs]


class KeyCase:
    """One layer's inputs: q [B,Hq,S,D] in the compute dtype's representation; the stored keys quantised to (kq, ks), their
    integer codes as float64 ``kint``. ``vq`` / ``vs`` / ``kinds`` alias the key side so that
    ``tests.gpu_harness.device_stores`` can put the case into guarded device stores."""

    def __init__(self, family, dtype, kind, q, k, info=None):
        self.family, self.dtype, self.kind, self.info = family, dtype, kind, info or {}
        self.q = q
        self.B, self.Hq, self.S, self.D = q.shape
        self.Hkv, self.T = k.shape[1], k.shape[2]
        self.sm = 1.0 / np.sqrt(self.D)
        kq, _, ks = O.quantize_tokens(k[None], kind, dtype="bf16" if dtype == "bf16" else None)
        self.kq, self.ks = kq[0], ks[0]
        self.kint = _codes(self.kq, kind, self.D)
        self.vq, self.vs, self.kinds = self.kq, self.ks, (kind, kind)

    @property
    def shape(self):
        return (self.B, self.Hq, self.Hkv, self.T, self.S, self.D)

    def reference(self):
        return key_mass(self)


def key_mass(c, **mistake):
    """float64 ``mass`` [B,Hkv,T] of case ``c``: :func:`key_mass_stored` of the case's own query, codes and scales."""
    return key_mass_stored(c.q, c.kint, c.ks, c.dtype, c.sm, **mistake)


def stored_codes(kq, kind, D):
    """integer codes of a store ``[B,Hkv,T,Dq]`` as float64 ``[B,Hkv,T,D]``: the ``kint`` :func:`key_mass_stored` takes"""
    return _codes(kq, kind, D)


def key_mass_stored(q, kint, ks, dtype, sm, shift=0, drop=(), norm_all=False, headmap="group", skip_head=None, scale_next=False,
                    swap_nibbles=False, prior=None, overwrite=False, values="exact"):
    """float64 ``mass`` [B,Hkv,T] from a store's own contents: ``q`` [B,Hq,S,D] in the representation of the compute dtype
    ``dtype``, ``kint`` float64 [B,Hkv,T,D] integer codes, ``ks`` [T] stored scales. ``prior`` [B,Hkv,T]: what ``mass`` held
    before an accumulating call.

    One deliberate mistake at a time: ``shift`` = +-1: the causal bound moved (row s sees t <= T - S + s + shift);
    ``drop``: stored tokens left out (of every row's softmax and of the result); ``norm_all``: the normaliser taken over all T
    keys instead of the visible ones; ``headmap="mod"``: query head h reads kv head h % Hkv (its mass still lands in
    h // nq); ``skip_head`` = j: head j of every group left out of the sum; ``scale_next``: ``k_scales[t + 1]`` used for t
    (the last token keeps its own); ``swap_nibbles``: the two codes of every byte of a packed INT4 row exchanged;
    ``overwrite``: an accumulating call that overwrites. ``values="rounded"``: the dequantised keys rounded to the compute
    dtype first (what the model deliberately does not do)."""
    B, Hq, S, D = q.shape
    Hkv, T = kint.shape[1], kint.shape[2]
    nq = Hq // Hkv
    ks = np.asarray(ks).astype(np.float64)
    if scale_next:
        ks = np.concatenate([ks[1:], ks[-1:]])
    if swap_nibbles:
        kint = kint.reshape(B, Hkv, T, D // 2, 2)[..., ::-1].reshape(B, Hkv, T, D)
    kd = kint * ks[:, None]
    if values == "rounded":
        kd = widen(narrow(kd, dtype), dtype)
    q = widen(q, dtype)
    t = np.arange(T)[None, :]
    vis = t <= (T - S + np.arange(S))[:, None] + shift
    for d_ in drop:
        vis[:, d_] = False
    mass = np.zeros((B, Hkv, T))
    for b in range(B):
        for h in range(Hq):
            g = h // nq
            if skip_head is not None and h - g * nq == skip_head:
                continue
            sc = q[b, h] @ kd[b, g if headmap == "group" else h % Hkv].T * sm  # [S,T]
            m = np.where(vis, sc, -np.inf).max(axis=1, keepdims=True)
            e = np.exp(sc - m)
            den = (e if norm_all else np.where(vis, e, 0.0)).sum(axis=1, keepdims=True)
            mass[b, g] += np.where(vis, e / den, 0.0).sum(axis=0)
    if prior is not None and not overwrite:
        mass = np.asarray(prior, np.float64) + mass
    return mass


def limit(ref, dtype):
    """the suite's standard tolerance, per element (tests.gpu_harness.within_standard)"""
    return TOL[dtype] * (np.abs(ref) + np.abs(ref).max())


def probe_targets(T, S):
    """the fixed probe targets of the ``probe`` family that exist at (T, S)"""
    return sorted({t for t in (0, 63, 64, T - S - 1, T - S, T - 1) if 0 <= t < T})


def make_case(family, B, Hq, Hkv, T, S, D, kind, dtype, seed=0):
    assert family in FAMILIES and 1 <= S <= T and Hq % Hkv == 0
    rng = np.random.default_rng(seed)
    nq = Hq // Hkv
    info = {}
    if family == "flat":
        k = rng.standard_normal((B, Hkv, T, D))
        q = rng.standard_normal((B, Hq, S, D))
    elif family == "scale_span":
        k = rng.standard_normal((B, Hkv, T, D)) * 10.0 ** rng.uniform(-4.0, 0.0, T)[None, None, :, None]
        q = rng.standard_normal((B, Hq, S, D)) * 2.0
    else:
        H, sq = hadamard(D), np.sqrt(D)
        k = rng.standard_normal((B, Hkv, T, D)) * 0.1
        q = rng.standard_normal((B, Hq, S, D)) * 0.5  # a row left without a direction keeps this
        fixed = probe_targets(T, S)
        dirs, aimed, n_fixed = {}, {}, 0  # aimed[(b, g, token)] = rows that point at it and see it
        blind = {}  # blind[(b, g)] = rows that point at a token they do not see: their weight spreads over what they see
        for i, (b, h, s) in enumerate((b, h, s) for b in range(B) for s in range(S) for h in range(Hq)):
            g, p = h // nq, T - S + s
            seen = [t_ for t_ in fixed if t_ <= p]
            choice = i % 4
            if choice == 1:
                tok = p  # its own position
            elif choice == 2 and s < S - 1:
                tok = p + 1  # one past the row: it must receive nothing from it
            else:
                tok = seen[n_fixed % len(seen)]
                n_fixed += 1
            key = (b, g, tok)
            if key not in dirs:
                used = sum(1 for k_ in dirs if k_[:2] == (b, g))
                if used >= D - 2:
                    continue
                amp = 1.0 + 2.0 * (tok % 2)  # adjacent targets: x1 / x3, so that a neighbour's scale moves the probe
                dirs[key] = (H[2 + used], amp)
                k[b, g, tok] += amp * H[2 + used]
            d_, amp = dirs[key]
            q[b, h, s] = 18.0 / (amp * sq) * d_
            if tok <= p:
                aimed[key] = aimed.get(key, 0) + 1
            else:
                blind[(b, g)] = blind.get((b, g), 0) + 1
        info = dict(aimed=aimed, blind=blind, fixed=fixed)
    return KeyCase(family, dtype, kind, narrow(q, dtype), narrow(k, dtype), info)


# (B, Hq, Hkv, T, S): every group size 1 / 4 / 5 / 16, S * nq at 63 / 64 / 65 (one query block, and one row into a second),
# S at 1 / 16 / 17, T at S, 63 / 64 / 65 and 319 / 320 / 321 (one tile, one token into a second; several splits), two batch
# rows with two kv heads
SHAPES = (
    (1, 4, 1, 1, 1),
    (1, 1, 1, 63, 1),
    (1, 4, 1, 64, 16),
    (1, 5, 1, 65, 13),
    (1, 16, 1, 17, 17),
    (2, 8, 2, 319, 16),
    (1, 7, 1, 320, 9),
    (2, 4, 2, 321, 17),
)
# several pass-1 splits and several query blocks (D = 128 in the issue's example; both head dims run it)
SHAPE_SPLITS_BLOCKS = (1, 8, 2, 1300, 40)
# pass-2 runs of two tiles: more than 1,024 (tile, batch row, kv head) triples
SHAPE_RUNS = (4, 8, 8, 2117, 3)


def np_keep_top_scores(scores, budget, prefix_len=0, recent=0, pool=1):
    """numpy restatement of cache.implementations.keep_indices_top_scores: a list of positions, or None (keep all)"""
    scores = np.asarray(scores, np.float32)
    T = len(scores)
    if budget >= T or prefix_len + recent >= T:
        return None
    r = pool // 2
    pooled = [scores[max(0, t - r):min(T, t + r + 1)].max() for t in range(T)]
    free = sorted(range(prefix_len, T - recent), key=lambda t: (-pooled[t], t))  # ties to the lower position
    return list(range(prefix_len)) + sorted(free[:budget - prefix_len - recent]) + list(range(T - recent, T))
