"""Inputs for the chunk summary inside the quantised store (kvq_store_chunk_pool, csrc/kvq_evict.hip), a CPU model of it and
numpy restatements of the mistakes such a kernel can make. numpy only: test_gpu_store_evict.py feeds the cases to both
kernels and compares codes and scale words bit for bit, test_store_evict_discrimination.py shows on the CPU that the cases
reject the mistakes.

A case is a dict: q [G,B,H,T,Dq] (int8, or uint8 packed INT4), s [G,T] fp32 (stored scales, exactly representable in
`dtype`), kind, dtype ("f16" | "bf16"), D, chunk, keep. The model is the composition of the oracle's own functions:
dequantize_tokens -> chunk_summarize_kv -> quantize_tokens for the pooled rows, the raw input for the kept tail.

Families
  order       two chunk rows with a large scale hold +c and -c in every column, the rows between hold small values: while
              the large value sits in the fp32 accumulator the small ones are partly absorbed, so the order of the sum
              decides the low bits that are left after the cancellation, and with them the stored code.
  rounding    full-width significands in every scale, so that float(code) * scale is not a value of `dtype`, and chunk means
              that land between `dtype` values.
  scale_span  per-token scales log-uniform over four decades inside every chunk; tail codes stay below QMAX (a requantised
              tail token then gets another scale).
  zero        chunks of zero codes only (amax = 0: the eps scale), the first and the ragged last one among them.
  extremes    +QMAX and QMIN in every head of every token.
  ragged      a last chunk of 1 token and of chunk - 1 tokens, chunk no power of two.
  nonfinite   what a poisoned token leaves in the store (code 0, scale NaN or +inf) inside pooled chunks and in the kept tail:
              the chunk's summary token is code 0 under a NaN scale (the mean of a NaN is a NaN: the composition quantises a
              slice that holds one), the tail tokens move with their raw bits, the clean chunks are what they were. Not in
              CASES: its scale words are compared by quant_cases.float_mismatch (NONFINITE_CASES, test_gpu_store_evict.py).
"""
import numpy as np

from oracle import kvq_oracle as O

QMAX = {"int8": 127, "int4": 7}
QMIN = {"int8": -127, "int4": -8}
EPS = 1e-8


def odt(dtype):
    return "bf16" if dtype == "bf16" else None


def to_storage(x32, dtype):
    x32 = np.asarray(x32, dtype=np.float32)
    return x32.astype(np.float16) if dtype == "f16" else O.f32_to_bf16_bits(x32)


def widen(x, dtype):
    return O._widen(x, odt(dtype))


def rt(x32, dtype):
    """fp32 -> dtype -> fp32"""
    return widen(to_storage(x32, dtype), dtype)


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def _key(kind, dtype):
    return (8 if kind == "int8" else 4, 16 if dtype == "f16" else 17)


def pack(codes, kind):
    """int codes [.., D] -> the store's bytes"""
    return codes.astype(np.int8) if kind == "int8" else O.pack_int4(codes.astype(np.int8))


def _codes(rng, kind, shape, lim=None):
    hi = QMAX[kind] if lim is None else lim
    lo = QMIN[kind] if lim is None else -lim
    return rng.integers(lo, hi + 1, size=shape)


def _scales(rng, dtype, shape, lo_exp, hi_exp):
    """random positive scales with a full-width significand, exactly representable in dtype"""
    p = 10 if dtype == "f16" else 7
    sig = 1.0 + rng.integers(0, 1 << p, size=shape).astype(np.float64) / float(1 << p)
    return rt((sig * np.exp2(rng.integers(lo_exp, hi_exp + 1, size=shape))).astype(np.float32), dtype)


def lengths(chunk, n_full, ragged, keep):
    old = n_full * chunk + ragged
    return old, old + keep


def _case(q, s, kind, dtype, D, chunk, keep):
    return dict(q=np.ascontiguousarray(q), s=np.ascontiguousarray(s, dtype=np.float32), kind=kind, dtype=dtype, D=D, chunk=chunk,
                keep=keep)


# ---------------------------------------------------------------------------------------------------------- families

def order(kind, dtype, chunk, G=2, B=1, H=2, D=64, n_full=3, ragged=0, keep=4, seed=0):
    assert chunk >= 3
    rng = _rng(seed, chunk, D, 1, *_key(kind, dtype))
    old, T = lengths(chunk, n_full, ragged, keep)
    codes = _codes(rng, kind, (G, B, H, T, D))
    s = _scales(rng, dtype, (G, T), -12, -7)
    for g in range(G):
        for c in range(n_full):
            r1 = int(rng.integers(0, chunk))
            r2 = (r1 + int(rng.integers(2, chunk))) % chunk  # never the same row, at least one row between
            # the largest binade in which QMAX * scale is still finite in fp16: ulp(fp32 sum) is 2^-9 .. 2^-8 while it holds
            # the large value, the size of the small values themselves
            big = float(_scales(rng, dtype, (1,), *((8, 8) if kind == "int8" else (12, 12)))[0])
            s[g, c * chunk + r1] = s[g, c * chunk + r2] = big
            col = rng.integers(QMAX[kind] // 2 + 1, QMAX[kind] + 1, size=(B, H, D))
            codes[g, :, :, c * chunk + r1] = col
            codes[g, :, :, c * chunk + r2] = -col
    return _case(pack(codes, kind), s, kind, dtype, D, chunk, keep)


def rounding(kind, dtype, chunk, G=2, B=1, H=2, D=64, n_full=3, ragged=0, keep=4, seed=0):
    rng = _rng(seed, chunk, D, 2, *_key(kind, dtype))
    _, T = lengths(chunk, n_full, ragged, keep)
    codes = _codes(rng, kind, (G, B, H, T, D))
    s = _scales(rng, dtype, (G, T), -3, -1)  # one binade spread: every row reaches the sum's low bits
    return _case(pack(codes, kind), s, kind, dtype, D, chunk, keep)


def scale_span(kind, dtype, chunk, G=2, B=2, H=2, D=64, n_full=3, ragged=0, keep=4, seed=0):
    rng = _rng(seed, chunk, D, 3, *_key(kind, dtype))
    old, T = lengths(chunk, n_full, ragged, keep)
    codes = _codes(rng, kind, (G, B, H, T, D))
    codes[:, :, :, old:] = _codes(rng, kind, (G, B, H, keep, D), lim=QMAX[kind] - 2)
    s = rt(np.power(10.0, rng.uniform(-3.0, 1.0, size=(G, T))).astype(np.float32), dtype)
    return _case(pack(codes, kind), s, kind, dtype, D, chunk, keep)


def zero(kind, dtype, chunk, G=2, B=1, H=2, D=64, n_full=3, ragged=0, keep=4, seed=0):
    rng = _rng(seed, chunk, D, 4, *_key(kind, dtype))
    old, T = lengths(chunk, n_full, ragged, keep)
    codes = _codes(rng, kind, (G, B, H, T, D))
    codes[:, :, :, :chunk] = 0
    codes[:, :, :, n_full * chunk:old] = 0
    if n_full >= 3:
        codes[0, :, :, 2 * chunk:3 * chunk] = 0
    s = _scales(rng, dtype, (G, T), -6, 0)
    return _case(pack(codes, kind), s, kind, dtype, D, chunk, keep)


def extremes(kind, dtype, chunk, G=2, B=1, H=2, D=64, n_full=3, ragged=0, keep=4, seed=0):
    rng = _rng(seed, chunk, D, 5, *_key(kind, dtype))
    _, T = lengths(chunk, n_full, ragged, keep)
    codes = _codes(rng, kind, (G, B, H, T, D))
    if D >= 2:
        d1 = rng.integers(0, D, size=(G, B, H, T, 1))
        d2 = (d1 + rng.integers(1, D, size=(G, B, H, T, 1))) % D
        np.put_along_axis(codes, d1, QMAX[kind], axis=4)
        np.put_along_axis(codes, d2, QMIN[kind], axis=4)
    s = _scales(rng, dtype, (G, T), -6, 0)
    return _case(pack(codes, kind), s, kind, dtype, D, chunk, keep)


def _divide_sensitive_sum(kind, dtype, chunk, pick):
    """A 24-bit integer N whose slice scale differs between N / chunk and N * (1 / chunk): N / chunk sits so close to the
    midpoint between two `dtype` values that the one-ulp error of the fp32 reciprocal product crosses it, and the pooled
    value is the slice's abs-max, so the crossing reaches the stored scale word. Found by search (pick: which hit)."""
    P = 11 if dtype == "f16" else 8
    M = np.arange((1 << P) + 1, 1 << (P + 1), 2, dtype=np.int64)  # odd P+1-bit integers: the midpoints
    j = np.arange(-4, 5, dtype=np.int64)
    t = 23 - np.floor(np.log2(chunk * M.astype(np.float64))).astype(np.int64)
    N = ((chunk * M) << t)[:, None] + j[None, :]
    N = N[(N >= 1 << 23) & (N < 1 << 24)]
    a = N.astype(np.float32) * np.float32(2.0 ** -14)  # exact
    m1 = rt(a / np.float32(chunk), dtype)
    m2 = rt(a * (np.float32(1.0) / np.float32(chunk)), dtype)
    s1, s2 = rt(m1 / np.float32(QMAX[kind]), dtype), rt(m2 / np.float32(QMAX[kind]), dtype)
    hits = N[s1 != s2]
    assert len(hits), (kind, dtype, chunk)
    return int(hits[pick % len(hits)])


def ragged(kind, dtype, chunk, last, G=2, B=1, H=2, D=64, n_full=2, keep=4, seed=0):
    """Chunk 0 of every group is built for the divide: column (b 0, h 0, d 0) sums EXACTLY to _divide_sensitive_sum() 2^-14
    (signed digits of that integer, one per row, under power-of-two scales; every partial sum is exact in fp32) and is the
    slice's abs-max (the other rows carry the scale 2^-14, the digit rows hold zero everywhere else)."""
    assert 1 <= last < chunk
    rng = _rng(seed, chunk, D, 6, last, *_key(kind, dtype))
    _, T = lengths(chunk, n_full, last, keep)
    codes = _codes(rng, kind, (G, B, H, T, D))
    s = _scales(rng, dtype, (G, T), -4, 0)
    w, nd = (7, 4) if kind == "int8" else (4, 7)
    assert chunk >= nd
    for g in range(G):
        N = _divide_sensitive_sum(kind, dtype, chunk, int(rng.integers(0, 1 << 30)))
        digits, R = [], 1 << w
        for _ in range(nd):
            d = (N + R // 2) % R - R // 2
            digits.append(d)
            N = (N - d) // R
        assert N == 0
        s[g, :chunk] = np.float32(2.0 ** -14)
        codes[g, 0, 0, :chunk, 0] = 0
        for i, d in enumerate(reversed(digits)):  # most significant digit first
            codes[g, :, :, i] = 0
            codes[g, 0, 0, i, 0] = d
            s[g, i] = np.float32(2.0 ** (-14 + w * (nd - 1 - i)))
    return _case(pack(codes, kind), s, kind, dtype, D, chunk, keep)


def nonfinite(kind, dtype, chunk, G=2, B=1, H=2, D=64, n_full=3, ragged=0, keep=4, seed=0):
    """The rounding family's data with poisoned tokens: chunk 0 of group 0 and chunk 1 of group 1 hold a NaN-scale token,
    chunk 1 of group 0 (and a ragged last chunk of group 1) a +inf-scale one; the first two tail tokens have one each.
    Chunk 2 of group 0 and chunk 0 of group 1 are clean. A poisoned token's codes are 0, as the quantise kernels store it."""
    assert n_full >= 3 and keep >= 2
    case = rounding(kind, dtype, chunk, G=G, B=B, H=H, D=D, n_full=n_full, ragged=ragged, keep=keep, seed=seed)
    old, T = lengths(chunk, n_full, ragged, keep)
    q, s = case["q"], case["s"]
    zero = 0x88 if kind == "int4" else 0
    spots = [(0, chunk // 2, np.nan), (0, chunk + chunk - 1, np.inf), (1, chunk, np.nan), (0, old, np.nan), (0, old + 1, np.inf),
             (1, old, np.inf), (1, old + 1, np.nan)]
    if ragged:
        spots.append((1, n_full * chunk, np.inf))
    for g, t, v in spots:
        s[g, t] = np.float32(v)
        q[g, :, :, t].view(np.uint8)[...] = zero
    return case


FAMILIES = dict(order=order, rounding=rounding, scale_span=scale_span, zero=zero, extremes=extremes, ragged=ragged, nonfinite=nonfinite)

KIND_DTYPE = [(k, d) for k in ("int8", "int4") for d in ("f16", "bf16")]

# the cases both test files run, as (family, kwargs)
CASES = ([("order", dict(kind=k, dtype=d, chunk=c, ragged=r)) for k, d in KIND_DTYPE for c, r in ((16, 0), (64, 1))]
         + [("rounding", dict(kind=k, dtype=d, chunk=c, ragged=r, B=2, H=4)) for k, d in KIND_DTYPE for c, r in ((16, 1), (7, 0))]
         + [("scale_span", dict(kind=k, dtype=d, chunk=c, ragged=r)) for k, d in KIND_DTYPE for c, r in ((16, 1), (64, 0))]
         + [("zero", dict(kind=k, dtype=d, chunk=16, ragged=3)) for k, d in KIND_DTYPE]
         + [("extremes", dict(kind=k, dtype=d, chunk=16, ragged=1)) for k, d in KIND_DTYPE]
         + [("ragged", dict(kind=k, dtype=d, chunk=c, last=l)) for k, d in KIND_DTYPE for c in (7, 100) for l in (1, c - 1)])


NONFINITE_CASES = [("nonfinite", dict(kind=k, dtype=d, chunk=c, ragged=r, B=2, H=4)) for k, d in KIND_DTYPE for c, r in ((16, 1), (7, 0))]


def case_id(fam, kw):
    return fam + "-" + "-".join(f"{k}{v}" if k not in ("kind", "dtype") else str(v) for k, v in kw.items())


def build(fam, kw):
    return FAMILIES[fam](**kw)


# ------------------------------------------------------------------------------------------------------------- model

def model(case):
    """kvq_store_chunk_pool from the oracle's own functions -> (codes [G,B,H,Tout,Dq], scales [G,Tout] fp32)"""
    q, s, kind, dtype, D, chunk, keep = (case[k] for k in ("q", "s", "kind", "dtype", "D", "chunk", "keep"))
    T = q.shape[3]
    k = min(keep, T)
    old = T - k
    if old <= 0:
        return q.copy(), s.copy()
    n = (old + chunk - 1) // chunk
    x = O.dequantize_tokens(q, s, kind, D, dtype)
    y = O.chunk_summarize_kv(x, chunk, keep, dtype=odt(dtype))
    q2, _, s2 = O.quantize_tokens(np.ascontiguousarray(y[:, :, :, :n]), kind, EPS, dtype=odt(dtype))
    return np.concatenate([q2.view(q.dtype), q[:, :, :, old:]], axis=3), np.concatenate([s2.astype(np.float32), s[:, old:]], axis=1)


def model_twice(case):
    """the reference loop re-summarises what it summarised: the model applied to its own output"""
    q1, s1 = model(case)
    return model(dict(case, q=q1, s=s1))


# ----------------------------------------------------------------------------------------------------------- mutants

MISTAKES = {  # name -> (keyword arguments of mutant(), the family whose every case must reject it)
    "sum_reversed": (dict(how="reversed"), "order"),
    "sum_pairwise": (dict(how="pairwise"), "order"),
    "x_not_rounded": (dict(round_x=False), "rounding"),
    "mean_not_rounded": (dict(round_mean=False), "rounding"),
    "reciprocal": (dict(div="recip"), "ragged"),
    "divisor_n": (dict(div="n"), "ragged"),
    "absmax_one_head": (dict(amax="head"), "scale_span"),
    "absmax_one_batch_row": (dict(amax="batch"), "scale_span"),
    "scale_not_rounded": (dict(round_scale=False), "scale_span"),
    "tail_requantised": (dict(tail="requant"), "scale_span"),
    "nibbles_swapped": (dict(nibbles="swapped"), "scale_span"),  # INT4 cases only
}


def _sum(c, how):
    """fp32 sum over axis -2"""
    if how == "reversed":
        c = c[..., ::-1, :]
    if how == "pairwise":
        while c.shape[-2] > 1:
            if c.shape[-2] % 2:
                c = np.concatenate([c, np.zeros_like(c[..., :1, :])], axis=-2)
            c = (c[..., 0::2, :] + c[..., 1::2, :]).astype(np.float32)
        return c[..., 0, :]
    acc = np.zeros(c.shape[:-2] + c.shape[-1:], dtype=np.float32)
    for j in range(c.shape[-2]):
        acc = (acc + c[..., j, :]).astype(np.float32)
    return acc


def _quant(m, kind, dtype, amax, round_scale=True, nibbles="ok"):
    """m [G,B,H,n,D] fp32, amax [G,n] -> (codes as stored, scales fp32)"""
    s32 = np.maximum(amax.astype(np.float32) / np.float32(QMAX[kind]), np.float32(EPS)).astype(np.float32)
    codes = np.clip(np.rint(m / s32[:, None, None, :, None]), QMIN[kind], QMAX[kind]).astype(np.int8)
    if kind == "int4":
        codes = O.pack_int4(codes)
        if nibbles == "swapped":
            codes = ((codes << np.uint8(4)) | (codes >> np.uint8(4))).astype(np.uint8)
    return codes, (rt(s32, dtype) if round_scale else s32)


def mutant(case, how="seq", round_x=True, round_mean=True, div="true", amax="all", round_scale=True, tail="copy", nibbles="ok"):
    """The model restated with one switch per mistake; the defaults are the model itself (the discrimination test holds
    them to model())."""
    q, s, kind, dtype, D, chunk, keep = (case[k] for k in ("q", "s", "kind", "dtype", "D", "chunk", "keep"))
    G, B, H, T, _ = q.shape
    k = min(keep, T)
    old = T - k
    if old <= 0:
        return q.copy(), s.copy()
    n = (old + chunk - 1) // chunk
    codes = (O.unpack_int4(q, D) if kind == "int4" else q).astype(np.float32)
    x = (codes * s[:, None, None, :, None]).astype(np.float32)
    if round_x:
        x = rt(x, dtype)
    body = x[:, :, :, :old]
    pad = n * chunk - old
    if pad:
        body = np.concatenate([body, np.zeros((G, B, H, pad, D), dtype=np.float32)], axis=3)
    acc = _sum(body.reshape(G, B, H, n, chunk, D), how)
    if div == "true":
        m = acc / np.float32(chunk)
    elif div == "recip":
        m = acc * (np.float32(1.0) / np.float32(chunk))
    else:
        rows = np.minimum(chunk, old - np.arange(n) * chunk).astype(np.float32)
        m = acc / rows[:, None]
    m = m.astype(np.float32)
    if round_mean:
        m = rt(m, dtype)
    a = np.abs(m)
    am = a.max(axis=(1, 2, 4)) if amax == "all" else a[:, :, 0].max(axis=(1, 3)) if amax == "head" else a[:, 0].max(axis=(1, 3))
    q2, s2 = _quant(m, kind, dtype, am, round_scale, nibbles)
    qt, st = q[:, :, :, old:], s[:, old:]
    if tail == "requant" and k:
        xt = rt(x[:, :, :, old:], dtype)
        qt, st = _quant(xt, kind, dtype, np.abs(xt).max(axis=(1, 2, 4)))
    return np.concatenate([q2.view(q.dtype), qt.view(q.dtype)], axis=3), np.concatenate([s2, st], axis=1).astype(np.float32)


def differs(a, b):
    """at least one code byte or scale word differs"""
    return bool((a[0].view(np.uint8) != b[0].view(np.uint8)).any() or (a[1].view(np.uint32) != b[1].view(np.uint32)).any())
