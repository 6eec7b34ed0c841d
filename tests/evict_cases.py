"""Adversarial inputs for the eviction kernels (csrc/kvq_evict.hip) and numpy restatements of the mistakes such a kernel
can make. numpy only: the GPU tests (test_gpu_evict_edges.py) feed the cases to every route and compare with the oracle
bit for bit, test_evict_discrimination.py shows on the CPU that the cases reject the mistakes.

Arrays are in the oracle's representation: f16 -> np.float16, bf16 -> uint16 bit patterns, f32 -> np.float32, shaped
[G, B, H, T, D] with T = n_full * chunk + ragged + keep (n_full whole chunks, a ragged last chunk, the kept tail).

Families
  order          every (row, d) column of every whole chunk holds +big and -big at two random rows and small values of
                 many magnitudes elsewhere. While big sits in the fp32 accumulator the small values are partly absorbed
                 (ulp(big) is 2^-9 at big = m 2^14), so WHICH rows are added in between decides the sum's low bits, and
                 after the exact cancellation nothing large is left to hide them from the final rounding to 16 bits.
  division       plain f32 data: the fp32 result is stored unrounded, so x * (1/c) and x / c differ for c no power of two.
  denormal_mean  sums that are exact in fp32 whose mean lands between 16-bit values, ties among them (f16: subnormal
                 results); chunks of -0.0 only (+0.0), with +inf (+inf) and whose fp32 sum overflows (+inf). Never NaN.
  ragged_tail    the kept rows right behind a short last chunk hold 65504, NaN and inf: reading past `old` shows.
  bits           every 16-bit pattern exactly once (f32: 65,536 words of specials and random bits) for the copy paths.
"""
import numpy as np

from oracle import kvq_oracle as O

DTYPES = ("f16", "bf16", "f32")
SIG_BITS = {"f16": 11, "bf16": 8, "f32": 24}
# order: exponent of big, lowest and highest exponent of the small values
ORDER_EXP = {"f16": (14, -14, -5), "bf16": (20, -10, 0), "f32": (14, -14, -5)}
# head_dim -> lane groups of chunk_pool_wave_k; (D, chunk) of its six <G, RPG> instantiations
WAVE_GROUPS = {256: 2, 128: 4, 64: 8}
WAVE_SHAPES = ((128, 64), (128, 32), (64, 64), (64, 128), (256, 32), (256, 16))
VEC_SHAPES = ((64, 7), (64, 24), (64, 40))          # chunk_pool_vec_k: less than a load batch, batches plus a remainder
GENERIC_SHAPES = ((5, 7, False), (128, 24, True))    # chunk_pool_generic_k: (D, chunk, misaligned slice)
POLICY_SHAPE = (4, 128, 64)                          # (G, D, chunk) of the Python-layer test: two layers of K and V
# every `order` case the GPU tests run, as order()'s arguments: test_evict_discrimination.py holds each to its condition
ORDER_CASES = ([dict(dtype=dt, chunk=c, D=D, ragged=1) for dt in DTYPES for D, c in WAVE_SHAPES + VEC_SHAPES if dt != "f32" or (D, c) in VEC_SHAPES]
               + [dict(dtype="f32", chunk=64, D=128, ragged=1)]
               + [dict(dtype=dt, chunk=c, D=D, ragged=1) for dt in DTYPES for D, c, _ in GENERIC_SHAPES]
               + [dict(dtype=dt, chunk=POLICY_SHAPE[2], G=POLICY_SHAPE[0], D=POLICY_SHAPE[1], ragged=1) for dt in ("f16", "bf16")])


def odt(dtype):
    """the oracle's dtype argument (tests.util.odt restated: that module imports torch, this one must not)"""
    return "bf16" if dtype == "bf16" else None


def to_storage(x32, dtype):
    """fp32 -> storage representation, RN-even"""
    x32 = np.asarray(x32, dtype=np.float32)
    if dtype == "f32":
        return x32.copy()
    if dtype == "f16":
        with np.errstate(over="ignore"):
            return x32.astype(np.float16)
    return O.f32_to_bf16_bits(x32)


def widen(x, dtype):
    return O._widen(x, odt(dtype))


def _signif(rng, shape, dtype):
    """random significands in [1, 2) that use the type's full width"""
    p = SIG_BITS[dtype] - 1
    return (1.0 + rng.integers(0, 1 << p, size=shape).astype(np.float64) / float(1 << p)).astype(np.float32)


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def lengths(chunk, n_full, ragged, keep):
    old = n_full * chunk + ragged
    return old, old + keep


# ---------------------------------------------------------------------------------------------------------- families

def order(dtype, chunk, G=2, B=1, H=2, D=64, n_full=3, ragged=0, keep=4, seed=0):
    big_e, lo, hi = ORDER_EXP[dtype]
    rng = _rng(seed, chunk, D, SIG_BITS[dtype], ragged)
    _, T = lengths(chunk, n_full, ragged, keep)
    shape = (G, B, H, T, D)
    x = _signif(rng, shape, dtype) * np.exp2(rng.integers(lo, hi + 1, size=shape)).astype(np.float32)
    x *= rng.choice(np.array([-1.0, 1.0], dtype=np.float32), size=shape)
    if chunk >= 2:
        for c in range(n_full):
            r1 = rng.integers(0, chunk, size=(G, B, H, 1, D))
            r2 = (r1 + rng.integers(1, chunk, size=(G, B, H, 1, D))) % chunk
            big = _signif(rng, (G, B, H, 1, D), dtype) * np.float32(2.0 ** big_e)
            blk = x[:, :, :, c * chunk:(c + 1) * chunk]
            np.put_along_axis(blk, r1, big, axis=3)
            np.put_along_axis(blk, r2, -big, axis=3)
    return to_storage(x, dtype)


def division(chunk, G=2, B=1, H=2, D=64, n_full=3, ragged=3, keep=4, seed=0):
    _, T = lengths(chunk, n_full, ragged, keep)
    return _rng(seed, chunk, D, 77).standard_normal((G, B, H, T, D), dtype=np.float32)


def ragged_tail(dtype, chunk, ragged, G=2, B=1, H=2, D=64, n_full=3, keep=4, seed=0):
    assert ragged >= 1 and keep >= 1
    old, T = lengths(chunk, n_full, ragged, keep)
    x = _rng(seed, chunk, D, ragged, 78).standard_normal((G, B, H, T, D), dtype=np.float32)
    poison = np.array([65504.0, np.nan, np.inf, -np.inf, -65504.0], dtype=np.float32)
    x[:, :, :, old:] = poison[(np.arange(keep)[:, None] + np.arange(D)[None, :]) % len(poison)]
    return to_storage(x, dtype)


def denormal_mean(dtype, chunk, G=2, B=1, H=2, D=64, ragged=0, keep=4, seed=0):
    """three whole chunks: [0] means between 16-bit values with planted ties; [1] columns of -0.0 only (d < D/2), the rest
    as [0]; [2] +inf in one row (d % 3 == 0), a sum that overflows fp32 where the type can (d % 3 == 1; f16: +inf
    again), the rest as [0]. The ragged rows and the tail are as [0] / random."""
    assert chunk >= 2
    n_full = 3
    old, T = lengths(chunk, n_full, ragged, keep)
    rng = _rng(seed, chunk, D, SIG_BITS[dtype], 79)
    shape = (G, B, H, T, D)
    x = np.where(rng.random(shape) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    col = (G, B, H, 1, D)
    for c in range(n_full + (1 if ragged else 0)):
        n = chunk if c < n_full else ragged
        blk = x[:, :, :, c * chunk:c * chunk + n]
        r1 = rng.integers(0, n, size=col)
        if dtype == "f16":
            # one value in [2^-14, 2^-8): a mean over 64 rows is an f16 subnormal. Every fourth column an exact tie of
            # the power-of-two chunks: odd * 2^-19 / 64 sits halfway between two multiples of 2^-24 (both parities)
            v = _signif(rng, col, dtype) * np.exp2(rng.integers(-14, -8, size=col)).astype(np.float32)
            tie = (2 * rng.integers(16, 32, size=col) + 1).astype(np.float32) * np.float32(2.0 ** -19)
            v = np.where(np.arange(D) % 4 == 0, tie, v).astype(np.float32)
            np.put_along_axis(blk, r1, v, axis=3)
        else:
            # a + b with b up to 2^-8 a: exact in fp32 and wider than the storage type; every fourth column b is half
            # an ulp of a, an exact tie (f32: the sum is stored as it is; the values sit at the subnormal boundary)
            e0 = -126 if dtype == "f32" else 0
            a = _signif(rng, col, "bf16") * np.exp2(rng.integers(e0, e0 + 6, size=col)).astype(np.float32)
            b = _signif(rng, col, "bf16") * np.exp2(np.floor(np.log2(a)) - 8 - rng.integers(0, 3, size=col)).astype(np.float32)
            b = np.where(np.arange(D) % 4 == 0, np.exp2(np.floor(np.log2(a)) - 8), b).astype(np.float32)
            np.put_along_axis(blk, r1, a, axis=3)
            if n >= 2:
                np.put_along_axis(blk, (r1 + rng.integers(1, n, size=col)) % n, b, axis=3)
    d = np.arange(D)
    x[:, :, :, chunk:2 * chunk, d < D // 2] = np.float32(-0.0)
    c2 = x[:, :, :, 2 * chunk:3 * chunk]
    rows = rng.integers(0, chunk, size=col)
    inf = np.where(d % 3 == 0, np.float32(np.inf), np.take_along_axis(c2, rows, axis=3)).astype(np.float32)
    np.put_along_axis(c2, rows, inf, axis=3)
    sel = d % 3 == 1
    if dtype == "f16":
        c2[:, :, :, 0, sel] = np.float32(np.inf)
    else:
        huge = O.bf16_bits_to_f32(np.array([0x7F7F], dtype=np.uint16))[0] if dtype == "bf16" else np.finfo(np.float32).max
        c2[:, :, :, 0, sel] = huge
        c2[:, :, :, chunk - 1, sel] = huge
    x[:, :, :, old:] = rng.standard_normal((G, B, H, keep, D), dtype=np.float32)
    with np.errstate(over="ignore"):
        return to_storage(x, dtype)


def bit_patterns(dtype, seed=0):
    """65,536 words in a seeded order. 16-bit types: every pattern exactly once. f32: +-0, +-inf, signalling and quiet
    NaNs with payloads, the smallest and largest subnormals and normals, then random words."""
    rng = _rng(seed, SIG_BITS[dtype], 80)
    if dtype != "f32":
        p = rng.permutation(1 << 16).astype(np.uint16)
        return p.view(np.float16) if dtype == "f16" else p
    special = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF,
               0x00800000, 0x80800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001,
               0x7FBFFFFF, 0xFFBFFFFF, 0x7FFFFFFF, 0xFFFFFFFF]
    nan_pay = rng.integers(1, 1 << 23, size=4096, dtype=np.uint32)          # both quiet and signalling, either sign
    nans = np.uint32(0x7F800000) | nan_pay | (rng.integers(0, 2, size=4096, dtype=np.uint32) << np.uint32(31))
    subn = rng.integers(1, 1 << 23, size=4096, dtype=np.uint32) | (rng.integers(0, 2, size=4096, dtype=np.uint32) << np.uint32(31))
    words = np.concatenate([np.array(special, dtype=np.uint32), nans, subn])
    words = np.concatenate([words, rng.integers(0, 1 << 32, size=(1 << 16) - len(words), dtype=np.uint64).astype(np.uint32)])
    return rng.permutation(words).view(np.float32)


def bits_case(dtype, seed=0):
    """(1, 1, 2, 64 + 256, 128), chunk 64, keep 256: 64 finite rows to pool, then the 65,536 patterns as the kept tail"""
    G, B, H, D, chunk, keep = 1, 1, 2, 128, 64, 256
    x = to_storage(_rng(seed, 81).standard_normal((G, B, H, chunk + keep, D), dtype=np.float32), dtype)
    x[:, :, :, chunk:] = bit_patterns(dtype, seed).reshape(G, B, H, keep, D)
    return x, chunk, keep


def bits_fill(shape, dtype, seed=0):
    """the patterns of bit_patterns() repeated over `shape`"""
    return np.resize(bit_patterns(dtype, seed), int(np.prod(shape))).reshape(shape)


# ----------------------------------------------------------------------------------------------------------- mutants

def _seq(rows, start=0.0):
    """sequential fp32 sum over axis -2"""
    acc = np.full(rows.shape[:-2] + rows.shape[-1:], start, dtype=np.float32)
    for j in range(rows.shape[-2]):
        acc = acc + rows[..., j, :]
    return acc


def _sum(c, how, dtype, groups):
    n = c.shape[-2]
    if how == "seq":
        return _seq(c)
    if how == "negzero":  # an accumulator that starts at -0.0
        return _seq(c, -0.0)
    if how == "reversed":
        return _seq(c[..., ::-1, :])
    if how == "swapped":  # rows 2i and 2i + 1 exchanged
        perm = np.arange(n) ^ 1
        perm[perm >= n] = n - 1
        return _seq(c[..., perm, :])
    if how == "pairwise":
        while c.shape[-2] > 1:
            if c.shape[-2] % 2:
                c = np.concatenate([c, np.zeros_like(c[..., :1, :])], axis=-2)
            c = c[..., 0::2, :] + c[..., 1::2, :]
        return c[..., 0, :]
    if how == "exact":  # float64 sum, rounded to fp32 once
        return c.astype(np.float64).sum(axis=-2).astype(np.float32)
    if how == "groups":  # every lane group sums its rows from zero, the partial sums are then combined in order
        assert n % groups == 0
        part = _seq(c.reshape(c.shape[:-2] + (groups, n // groups) + c.shape[-1:]))
        return _seq(part)
    if how == "lowp":  # accumulator kept in the storage type
        acc = np.zeros(c.shape[:-2] + c.shape[-1:], dtype=np.float32)
        for j in range(n):
            acc = widen(to_storage(acc + c[..., j, :], dtype), dtype)
        return acc
    raise ValueError(how)


def _round(v, dtype, mode):
    r = to_storage(v, dtype)
    if dtype == "f32" or mode == "rn":
        return r
    u = r.view(np.uint16).copy()
    if mode == "ftz":  # subnormal results flushed to a signed zero
        emask = 0x7C00 if dtype == "f16" else 0x7F80
        return _as(np.where((u & emask) == 0, u & 0x8000, u).astype(np.uint16), dtype)
    assert mode == "away"  # ties away from zero
    av = np.abs(v.astype(np.float64))
    finite = np.isfinite(av) & ((u & 0x7FFF) < (0x7C00 if dtype == "f16" else 0x7F80))
    over = finite & (np.abs(widen(r, dtype).astype(np.float64)) > av)
    down = np.where(over, u - 1, u).astype(np.uint16)
    up = (down + 1).astype(np.uint16)
    lo = np.abs(widen(_as(down, dtype), dtype).astype(np.float64))
    with np.errstate(invalid="ignore", over="ignore"):
        hi = np.abs(widen(_as(up, dtype), dtype).astype(np.float64))
        tie = finite & (lo != av) & np.isfinite(hi) & ((av - lo) == (hi - av))
    return _as(np.where(tie, up, u).astype(np.uint16), dtype)


def _as(u16, dtype):
    return u16.view(np.float16) if dtype == "f16" else u16


def count_ties(x, dtype, chunk, keep):
    """pooled outputs whose fp32 mean lies exactly halfway between two values of the storage type"""
    rn, away = pooled(x, dtype, chunk, keep), pooled(x, dtype, chunk, keep, rounding="away")
    return int((np.ascontiguousarray(rn).view(np.uint16) != np.ascontiguousarray(away).view(np.uint16)).sum())


def pooled(x, dtype, chunk, keep, how="seq", groups=None, div="true", ragged="stop", rounding="rn"):
    """The pooled rows [..., n_chunks, D] of chunk_summarize_kv in the storage representation. The defaults restate the
    oracle; every other argument value is one mistake:
      how      reversed / swapped / pairwise / exact / groups (with `groups` lane groups) / lowp / negzero
      div      recip (acc * (1/chunk)) / n (the ragged chunk divided by its own row count)
      ragged   overread (the ragged chunk reads `chunk` rows, on into the kept tail)
      rounding ftz / away"""
    T, D = x.shape[-2], x.shape[-1]
    keep = min(keep, T)
    old = T - keep
    n = (old + chunk - 1) // chunk
    x32 = widen(x, dtype)
    body = x32[..., :min(T if ragged == "overread" else old, n * chunk), :]
    pad = n * chunk - body.shape[-2]
    if pad:
        body = np.concatenate([body, np.zeros(body.shape[:-2] + (pad, D), dtype=np.float32)], axis=-2)
    with np.errstate(over="ignore", invalid="ignore"):
        acc = _sum(body.reshape(body.shape[:-2] + (n, chunk, D)), how, dtype, groups)
        if div == "true":
            v = acc / np.float32(chunk)
        elif div == "recip":
            v = acc * (np.float32(1.0) / np.float32(chunk))
        else:
            assert div == "n"
            rows = np.minimum(chunk, old - np.arange(n) * chunk).astype(np.float32)
            v = acc / rows[:, None]
        return _round(v.astype(np.float32), dtype, rounding)


def changed_share(a, b):
    """share of elements whose stored bits differ"""
    w = np.uint32 if a.dtype.itemsize == 4 else np.uint16
    return float((np.ascontiguousarray(a).view(w) != np.ascontiguousarray(b).view(w)).mean())
