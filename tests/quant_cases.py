"""Input families that reach the edges of the quantise arithmetic, and an exact emulation of the vector kernels' quotient.

The quantise contract is ``q = clamp(rint(x32 / s32), QMIN, QMAX)`` with ``s32 = max(amax / QMAX, eps)`` and an IEEE
fp32 division. The vector kernels do not divide: ``quotient_bits8`` (csrc/kvq_quant.hip) rounds ``x * RN(1/s32)`` with a
magic-number add and redoes an 8-element vector with the IEEE division when a product lies within
``kM = 1.5 * QMAX * 2^-22`` of a half-integer. Random N(0,1) data almost never reaches that guard, an exact tie, the
``eps`` floor or a clamp; the builders here do, on purpose:

  exhaustive_cases    every finite fp16 / bf16 value with |x| <= amax, for amax values that make s32 a power of two, three
                      times one, a full-significand value, the dtype's largest value, and one below QMAX * eps
  tie_cases           x = (k + 1/2) * s32 exactly, its 1-ulp neighbours and values on both sides of the guard threshold
  probe_cases         each token's maximum in a chosen (row, 16-byte vector, lane) with alternating sign
  eps_cases           eps = 0.25 (floors every token) and 1e-3 (floors some)
  table_cases         caller-given abs-max tables: equal, 1 ulp and 2x larger, 1/2 and 1 ulp smaller, zero for some tokens
  nonfinite_cases     NaN (quiet, negative, signalling pattern), +inf, -inf and their mixes in some tokens of Gaussian
                      data, at the positions probe_cases uses; caller-given tables over such data, and NaN / +inf entries
  dequant_code_cases  all 256 INT8 / packed INT4 bytes against scales with subnormal, overflowing, tie and +-0 products,
                      and NaN, +inf and -inf scales

The non-finite contract (the reference's own behaviour, pinned by tests/golden/g10_nonfinite.npz): a slice with a
non-finite element stores code 0 throughout and the scale NaN (a NaN in the slice) or +inf (an inf, no NaN); under a
caller-given finite scale ±inf clamps to QMAX / QMIN and NaN is code 0; a NaN or +inf table entry gives code 0 and that
scale. :func:`float_mismatch` is the comparison rule: where the reference has a NaN any NaN will do, everywhere else the
bits are compared (+inf is a value). :func:`contract_quant` states the rule slice by slice, with switches for the
mistakes a kernel can make with it.

Arrays are [G, B, H, T, D] in the oracle's representation (fp16 / fp32 numpy, bf16 as uint16 bits; ``tests/util.py``).
:func:`emulate_quant` restates ``quotient_bits8`` + ``pack_i8`` / ``pack_i4`` in exact arithmetic, with switches that
remove the fallback, the clamp or the fused rounding, or round half away from zero: the CPU tests in
``test_quant_discrimination.py`` use it to show that these families tell a correct kernel from a subtly wrong one.
No GPU imports: the CPU suite uses this module.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from oracle import kvq_oracle as O

F32 = np.float32
QMAX = {"int8": 127, "int4": 7}
QMIN = {"int8": -127, "int4": -8}
KINDS = ("int8", "int4")


@dataclass
class Case:
    name: str
    x: np.ndarray                  # [G, B, H, T, D] in the oracle's representation
    dtype: str                     # "f16" | "bf16" | "f32"
    eps: float = 1e-8
    table: np.ndarray | None = None  # [G, T] fp32 abs-max table given to the from_absmax entry point; None: the data's own
    tags: set = field(default_factory=set)


# ----------------------------------------------------------------------------------------------------- dtype helpers

def odt(dtype: str):
    return "bf16" if dtype == "bf16" else None


def to_dtype(v32: np.ndarray, dtype: str) -> np.ndarray:
    """fp32 values -> the oracle's representation of ``dtype`` (RN-even)."""
    v32 = np.asarray(v32, dtype=F32)
    if dtype == "f16":
        return v32.astype(np.float16)
    if dtype == "bf16":
        return O.f32_to_bf16_bits(v32)
    return v32


def widen(x: np.ndarray, dtype: str) -> np.ndarray:
    return O._widen(x, odt(dtype))


def exact_in(v32: np.ndarray, dtype: str) -> np.ndarray:
    """mask: the fp32 value is exactly representable in ``dtype`` (and finite)"""
    v32 = np.asarray(v32, dtype=F32)
    return np.isfinite(v32) & (widen(to_dtype(v32, dtype), dtype) == v32)


def finite_values(dtype: str) -> np.ndarray:
    """every finite value of a 2-byte dtype as fp32 (both zeros included)"""
    b = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    v = b.view(np.float16).astype(F32) if dtype == "f16" else O.bf16_bits_to_f32(b)
    return v[np.isfinite(v)]


def data_absmax(x: np.ndarray, dtype: str) -> np.ndarray:
    return O.absmax_tokens(x, odt(dtype))


def scale32(amax: np.ndarray, kind: str, eps: float) -> np.ndarray:
    return O._scale_f32(amax, QMAX[kind], eps)


# --------------------------------------------------------------------------------------------------------- layout

def lay_out(values: np.ndarray, amax: np.ndarray, shape, dtype: str, c: int = 5) -> np.ndarray:
    """[G,B,H,T,D] array: token n (= g*T + t) holds ``±amax[n]`` once, at row n mod R, element
    ``8 * ((n*c) mod D/8) + n mod 8`` (a position probe; D not a multiple of 8: (n*c) mod D), and ``values`` fill the
    other slots in order, cycling. ``values`` must be at most ``amax`` in magnitude for the scale to be the intended one."""
    G, B, H, T, D = shape
    R, n_tok, per = B * H, G * T, B * H * D
    amax = np.broadcast_to(np.asarray(amax, dtype=F32), (n_tok,))
    vals = np.asarray(values, dtype=F32)
    out = np.empty((n_tok, per), dtype=F32)
    idx = np.arange(n_tok * (per - 1)) % max(len(vals), 1)
    fill = vals[idx].reshape(n_tok, per - 1) if len(vals) else np.zeros((n_tok, per - 1), F32)
    n = np.arange(n_tok)
    row = n % R
    d = 8 * ((n * c) % (D // 8)) + n % 8 if D % 8 == 0 else (n * c) % D
    pos = row * D + d
    sign = np.where(n % 2 == 0, F32(1), F32(-1))
    for i in range(n_tok):
        out[i, :pos[i]] = fill[i, :pos[i]]
        out[i, pos[i]] = sign[i] * amax[i]
        out[i, pos[i] + 1:] = fill[i, pos[i]:]
    # token-major [G, T, B, H, D] -> [G, B, H, T, D]
    x = out.reshape(G, T, B, H, D).transpose(0, 2, 3, 1, 4)
    return to_dtype(np.ascontiguousarray(x), dtype)


def _chunks(values: np.ndarray, shape, max_chunks: int):
    """split ``values`` into at most ``max_chunks`` pieces that each fit one tensor of ``shape`` (one slot per token is
    the maximum); with more values than that, every chunk takes a strided subset so that all magnitudes are sampled."""
    G, B, H, T, D = shape
    cap = G * T * (B * H * D - 1)
    n = -(-len(values) // cap)
    if n <= max_chunks:
        return [values[i * cap:(i + 1) * cap] for i in range(n)]
    return [values[i::n][:cap] for i in range(max_chunks)]


# ---------------------------------------------------------------------------------------------------- the families

def amax_set(dtype: str, kind: str) -> list:
    """(label, amax) pairs of the exhaustive family, each exact in ``dtype``; see the module docstring."""
    qm = QMAX[kind]
    out = [("pow2", F32(4.0)),
           ("s_pow2", F32(qm * 2.0 ** -6)),          # s32 = 2^-6 exactly
           ("s_3pow2", F32(3 * qm * 2.0 ** -6)),     # s32 = 3 * 2^-6 exactly (381/64 for INT8)
           ("s_full", F32(2.0 ** -3 * 11)),           # 1.375 / QMAX: a full 24-bit significand
           ("largest", F32(65504.0) if dtype == "f16" else O.bf16_bits_to_f32(np.array([0x7F7F], np.uint16))[0]),
           ("eps_floor", F32(2.0 ** -21 if kind == "int8" else 2.0 ** -24))]  # below QMAX * 1e-8: s32 = eps; fp16 subnormals
    return [(n, a) for n, a in out if exact_in(np.array([a]), dtype)[0]]


def exhaustive_cases(shape, dtype: str, kind: str, max_chunks: int = 2) -> list:
    """Every finite value of the 2-byte ``dtype`` (an fp32 input takes the fp16 set) with |x| <= amax, over the tokens of
    ``shape``; every token carries ±amax once, so every token gets the intended scale. When the values do not fit
    ``max_chunks`` tensors of ``shape``, each chunk is a strided subset (every magnitude range sampled, not every value)."""
    src = "f16" if dtype == "f32" else dtype
    allv = finite_values(src)
    cases = []
    for label, a in amax_set(src, kind):
        vals = allv[np.abs(allv) <= a]
        for i, ch in enumerate(_chunks(vals, shape, max_chunks)):
            x = lay_out(ch, a, shape, dtype)
            cases.append(Case(f"exh_{label}_{i}", x, dtype, tags={"exhaustive", label}))
    return cases


def tie_values(s32: float, kind: str, dtype: str) -> np.ndarray:
    """For every k in [QMIN, QMAX): x = (k + 1/2) * s32 exactly (fp32), its ±1-ulp fp32 neighbours and the values whose
    product x * RN(1/s32) lies just inside and just outside the guard threshold |d| = 1/2 - kM. Values not exact in
    ``dtype`` are dropped (a 2-byte dtype keeps the exact ties of short-significand scales)."""
    s = F32(s32)
    r = F32(1) / s
    km = F32(1.5) * F32(QMAX[kind]) * F32(2.0 ** -22)
    thr = F32(0.5) - km
    k = np.arange(QMIN[kind], QMAX[kind], dtype=np.float64)
    tie = ((k + 0.5) * np.float64(s)).astype(F32)
    vals = [tie, np.nextafter(tie, F32(np.inf)), np.nextafter(tie, F32(-np.inf))]
    for kk in (k, k + 1):  # around every integer: the products k ± (1/2 - kM) and a few fp32 steps on each side
        for side in (-1, 1):
            target = (kk + side * np.float64(thr)) / np.float64(r)
            base = target.astype(F32)
            for step in range(-3, 4):
                v = base
                for _ in range(abs(step)):
                    v = np.nextafter(v, F32(np.inf) if step > 0 else F32(-np.inf))
                vals.append(v)
    v = np.concatenate(vals).astype(F32)
    v = v[np.abs(v) <= F32(QMAX[kind]) * s]
    v = v[exact_in(v, dtype)]
    return np.unique(v)


def tie_scales(kind: str, dtype: str) -> list:
    """(label, amax, eps): s32 = 2^-6, 3 * 2^-6, 5 * 2^-8 from amax = QMAX * s32, and full-significand s32, with amax
    exact in ``dtype``; and s32 = eps = 3 * 2^-10 on the eps floor, which gives a 2-byte dtype exact ties against an
    inexact reciprocal even where QMAX * 3 * 2^e is not representable (bf16 at INT8)."""
    qm = QMAX[kind]
    out = [("s_pow2", F32(qm * 2.0 ** -6), 1e-8), ("s_3pow2", F32(3 * qm * 2.0 ** -6), 1e-8),
           ("s_5pow2", F32(5 * qm * 2.0 ** -8), 1e-8), ("s_full", F32(1.375), 1e-8), ("s_full2", F32(2.0 ** 3 * 1.8125), 1e-8),
           ("eps_3pow2", None, float(F32(3 * 2.0 ** -10)))]
    return [(n, a, e) for n, a, e in out if a is None or exact_in(np.array([a]), dtype)[0]]


def tie_cases(shape, dtype: str, kind: str) -> list:
    cases = []
    for label, a, eps in tie_scales(kind, dtype):
        s = F32(eps) if a is None else scale32(np.array([a]), kind, eps)[0]
        vals = tie_values(s, kind, dtype)
        if len(vals) == 0:
            continue
        if a is None:  # on the eps floor: the largest value stays below QMAX * eps
            a = np.abs(vals).max()
        for i, ch in enumerate(_chunks(vals, shape, 2)):
            cases.append(Case(f"tie_{label}_{i}", lay_out(ch, a, shape, dtype), dtype, eps=eps, tags={"ties", label}))
    return cases


def probe_cases(shape, dtype: str, seed: int = 2) -> list:
    """Position probes: token n's maximum (log-uniform in [2^-4, 2^6], rounded to the dtype) at (row n mod R, vector
    (n*c) mod D/8, lane n mod 8) with alternating sign; every other value at most amax/2. Two strides c = 5 and 3, so
    that with enough tokens every row, vector slot and lane holds some token's maximum."""
    G, B, H, T, D = shape
    rng = np.random.default_rng(seed)
    cases = []
    for c in (5, 3):
        n_tok = G * T
        amax = widen(to_dtype(np.exp2(rng.uniform(-4, 6, n_tok)).astype(F32), dtype), dtype)
        x = lay_out(np.zeros(1, F32), amax, shape, "f32", c=c)
        rest = rng.uniform(-0.5, 0.5, x.shape).astype(F32) * amax.reshape(G, 1, 1, T, 1)
        rest = widen(to_dtype(rest, dtype), dtype)  # rounding keeps |v| <= amax / 2
        x = np.where(x != 0, x, rest)
        cases.append(Case(f"probe_c{c}", to_dtype(x, dtype), dtype, tags={"probe"}))
    return cases


def eps_cases(shape, dtype: str, seed: int = 3) -> list:
    """Per-token maxima log-spread over [1e-4, 1.7]: eps = 0.25 floors every token of either kind (7 * 0.25 = 1.75),
    eps = 1e-3 the tokens with amax < QMAX * 1e-3."""
    G, B, H, T, D = shape
    rng = np.random.default_rng(seed)
    n_tok = G * T
    amax = widen(to_dtype(np.exp2(rng.uniform(np.log2(1e-4), np.log2(1.7), n_tok)).astype(F32), dtype), dtype)
    amax[::3] = widen(to_dtype(np.exp2(rng.uniform(np.log2(1e-4), np.log2(0.5), len(amax[::3]))).astype(F32), dtype), dtype)
    vals = rng.uniform(-1, 1, (G * T, B * H * D)).astype(F32) * amax[:, None]
    vals = widen(to_dtype(vals, dtype), dtype)
    x = vals.reshape(G, T, B, H, D).transpose(0, 2, 3, 1, 4)
    x = np.ascontiguousarray(x)
    out = []
    for eps in (0.25, 1e-3):
        out.append(Case(f"eps_{eps:g}", to_dtype(x, dtype), dtype, eps=eps, tags={"eps"}))
    return out


def table_cases(shape, dtype: str, seed: int = 4) -> list:
    """Caller-given abs-max tables over N(0,1)-like data with outliers: the data's own maximum, 1 fp32 ulp and 2x larger,
    1/2 and 1 ulp smaller (the clamp fires; INT4 reaches -8 and nibble 0), and zero for every third token (the eps
    floor: every nonzero value clamps)."""
    G, B, H, T, D = shape
    rng = np.random.default_rng(seed)
    x32 = rng.standard_normal(shape).astype(F32)
    x32[..., ::7] *= 4
    x = to_dtype(x32, dtype)
    am = data_absmax(x, dtype)
    zero = am.copy()
    zero[:, ::3] = 0
    tabs = [("equal", am), ("ulp_up", np.nextafter(am, F32(np.inf))), ("double", am * F32(2)),
            ("half", am * F32(0.5)), ("ulp_down", np.nextafter(am, F32(0))), ("zero", zero)]
    return [Case(f"table_{n}", x, dtype, table=t.astype(F32), tags={"table", n}) for n, t in tabs]


# ------------------------------------------------------------------------------------------------ non-finite inputs

UINT = {"f16": np.uint16, "bf16": np.uint16, "f32": np.uint32}
INF_BITS = {"f16": 0x7C00, "bf16": 0x7F80, "f32": 0x7F800000}
SIGN_BIT = {"f16": 0x8000, "bf16": 0x8000, "f32": 0x80000000}
QUIET_BIT = {"f16": 0x0200, "bf16": 0x0040, "f32": 0x00400000}
POISONS = ("qnan", "neg_nan", "snan", "pinf", "ninf", "both_inf", "nan_inf")


def poison_bits(dtype: str, poison: str) -> list:
    """The bit patterns a poison puts into one slice (one or two elements). ``snan`` is the pattern one above inf: the
    smallest NaN by its bits, which an integer maximum of patterns ranks just above inf and a value maximum drops."""
    inf, sign = INF_BITS[dtype], SIGN_BIT[dtype]
    one = {"qnan": inf | QUIET_BIT[dtype], "neg_nan": sign | inf | QUIET_BIT[dtype], "snan": inf + 1, "pinf": inf,
           "ninf": sign | inf}
    if poison == "both_inf":
        return [one["pinf"], one["ninf"]]
    if poison == "nan_inf":  # NaN must win wherever it stands: the inf comes first in memory here, last in the next token
        return [one["pinf"], one["snan"]]
    return [one[poison]]


def raw_bits(a: np.ndarray, dtype: str) -> np.ndarray:
    """unsigned view of an array in the oracle's representation"""
    return np.ascontiguousarray(a).view(UINT[dtype])


def is_nan_bits(u: np.ndarray, dtype: str) -> np.ndarray:
    return (u & (SIGN_BIT[dtype] - 1)) > INF_BITS[dtype]


def float_mismatch(got: np.ndarray, ref: np.ndarray, dtype: str) -> np.ndarray:
    """The comparison rule for scales and float outputs, position by position: where ``ref`` holds a NaN, ``got`` must hold
    a NaN of any sign and payload (x86 numpy and the GPU make different default NaNs and the reference fixes neither);
    everywhere else the bits must be equal. Returns the mask of positions that break the rule."""
    g, r = raw_bits(got, dtype), raw_bits(ref, dtype)
    assert g.shape == r.shape, (g.shape, r.shape)
    rn = is_nan_bits(r, dtype)
    return np.where(rn, ~is_nan_bits(g, dtype), g != r)


def same_floats(got, ref, dtype: str = "f32") -> bool:
    return not float_mismatch(np.asarray(got), np.asarray(ref), dtype).any()


def slice_positions(shape) -> list:
    """(row, element) of a [B*H, D] slice where a poison goes, as probe_cases places its maxima, so that every partition
    of an abs-max reduction meets one: the slice's first and last element (the first and last 8,192-element piece of the
    decode step's parts routine), a middle row at the first lane of a 16-byte vector, the last batch row at the last lane
    of one, and both lanes in the last and first row."""
    G, B, H, T, D = shape
    R = B * H
    v = (D // 8) // 2 * 8 if D >= 8 else 0          # a vector in the middle of the row
    last = min(v + 7, D - 1)
    pos = [(0, 0), (R - 1, D - 1), (R // 2, v), ((B - 1) * H, last), (R - 1, v), (0, last)]
    return pos


def poisoned_tokens(T: int, i: int) -> list:
    """Tokens 0, T - 1 and one in the middle, their neighbours clean. T of 3 or 4 leaves no clean token between three
    poisoned ones, so every other case (odd ``i``) poisons the two ends only; T < 3: one token, case ``i`` picks it."""
    if T >= 5:
        return [0, T // 2, T - 1]
    if T >= 3:
        return [0, T // 2, T - 1] if i % 2 == 0 else [0, T - 1]
    return [i % T]


def gaussian_base(shape, dtype: str, seed: int = 5) -> np.ndarray:
    x32 = np.random.default_rng(seed).standard_normal(shape).astype(F32)
    return to_dtype(x32, dtype)


def poison(x: np.ndarray, dtype: str, shape, name: str, i: int, tokens=None) -> np.ndarray:
    """A copy of ``x`` with poison ``name`` in ``tokens`` (default: poisoned_tokens) of every group; the n-th poisoned
    slice takes position (n + i) of slice_positions, a two-element poison that and the next one (swapped every other
    slice, so that each element leads once)."""
    G, B, H, T, D = shape
    out = np.ascontiguousarray(x).copy()
    u = out.view(UINT[dtype]).reshape(G, B * H, T, D)
    pos = slice_positions(shape)
    pats = poison_bits(dtype, name)
    n = i
    for g in range(G):
        for t in (poisoned_tokens(T, i) if tokens is None else tokens):
            pp = pats if n % 2 == 0 else pats[::-1]
            for k, b in enumerate(pp):
                r, d = pos[(n + k) % len(pos)]
                if B * H * D == 1:
                    r = d = 0
                u[g, r, t, d] = b
            n += 1
    return out


def nonfinite_cases(shape, dtype: str, kind: str, given_table: bool) -> list:
    """One case per poison over the Gaussian base data of ``shape`` (module docstring). A slice past 8,192 elements adds
    two cases for the decode step's parts routine: the only poison of the tensor in the first piece of token 0, and in
    the last piece of the last token. ``given_table`` adds finite tables over poisoned data (the clean data's maximum,
    half of it: below the data, and zero for every third token: the eps floor) and NaN / +inf entries over clean data."""
    G, B, H, T, D = shape
    base = gaussian_base(shape, dtype)
    cases = [Case(f"nonfinite_{name}", poison(base, dtype, shape, name, i), dtype, tags={"nonfinite", name})
             for i, name in enumerate(POISONS)]
    if B * H * D > 8192:
        u = [np.ascontiguousarray(base).copy() for _ in range(2)]
        u[0].view(UINT[dtype]).reshape(G, B * H, T, D)[0, 0, 0, 0] = poison_bits(dtype, "snan")[0]
        u[1].view(UINT[dtype]).reshape(G, B * H, T, D)[G - 1, B * H - 1, T - 1, D - 1] = poison_bits(dtype, "ninf")[0]
        cases += [Case("nonfinite_piece_first", u[0], dtype, tags={"nonfinite", "piece"}),
                  Case("nonfinite_piece_last", u[1], dtype, tags={"nonfinite", "piece"})]
    if given_table:
        am = data_absmax(base, dtype)
        zero = am.copy()
        zero[:, ::3] = 0
        i = 0
        for tname, tab in (("equal", am), ("below", am * F32(0.5)), ("zero", zero)):
            for name in ("snan", "neg_nan", "both_inf", "nan_inf"):
                cases.append(Case(f"nonfinite_table_{tname}_{name}", poison(base, dtype, shape, name, i), dtype,
                                  table=tab.astype(F32), tags={"nonfinite", "table", tname, name}))
                i += 1
        for ename, val in (("nan", F32(np.nan)), ("inf", F32(np.inf))):
            tab = am.copy()
            tab[:, poisoned_tokens(T, i)] = val
            cases.append(Case(f"nonfinite_entry_{ename}", base, dtype, table=tab, tags={"nonfinite", "table", "entry", ename}))
            i += 1
    return cases


def absmax_class(am: np.ndarray) -> np.ndarray:
    """0 finite, 1 +inf, 2 NaN, per entry of an abs-max table"""
    return np.where(np.isnan(am), 2, np.where(np.isinf(am), 1, 0))


def contract_quant(case: Case, kind: str, *, drop_nan=False, eps_swallows_nan=False, nan_as_qmin=False, nibble_zero=False,
                   leak=False):
    """(q, scales_f32) by the non-finite contract, stated slice by slice and independently of the oracle's arithmetic on
    such values; finite slices take the oracle. Switches, one per mistake a kernel can make:
      drop_nan          the abs-max is a value maximum that drops a NaN (fmaxf): the scale comes from the other elements
      eps_swallows_nan  max(amax / QMAX, eps) with an fmaxf: a NaN abs-max becomes eps
      nan_as_qmin       clamp(rint(NaN)) through fmaxf / fminf: a NaN quotient is stored as QMIN
      nibble_zero       INT4: the byte of a non-finite magic sum is 0, nibble 0 = code -8, where the reference stores 8
      leak              a poisoned token's abs-max also enters its right neighbour's"""
    G, B, H, T, D = case.x.shape
    x32 = widen(case.x, case.dtype)
    qm, qn = F32(QMAX[kind]), F32(QMIN[kind])
    codes = np.zeros(x32.shape, np.int8)
    nanq = np.zeros(x32.shape, bool)                    # elements whose quotient is a NaN
    s32 = np.zeros((G, T), F32)
    for g in range(G):
        carry = None
        for t in range(T):
            sl = x32[g, :, :, t, :]
            if case.table is not None:
                am = F32(case.table[g, t])
            elif np.isnan(sl).any() and not drop_nan:
                am = F32(np.nan)
            else:
                am = np.abs(sl[~np.isnan(sl)]).max() if (~np.isnan(sl)).any() else F32(0)
            if leak and carry is not None:
                am = F32(np.nan) if np.isnan(carry) or np.isnan(am) else max(am, carry)
            carry = am if not np.isfinite(am) else None
            if np.isnan(am):
                s = F32(case.eps) if eps_swallows_nan else F32(np.nan)
            else:
                s = max(F32(am / qm), F32(case.eps))
            s32[g, t] = s
            if not np.isfinite(s):                      # every quotient is 0 (finite / inf) or NaN: code 0
                nanq[g, :, :, t, :] = ~np.isfinite(sl) | np.isnan(s)
                continue
            fin = np.isfinite(sl)
            with np.errstate(over="ignore", invalid="ignore"):
                r = np.clip(np.rint(np.where(fin, sl, F32(0)) / s), qn, qm)
            r = np.where(np.isposinf(sl), qm, np.where(np.isneginf(sl), qn, r))   # the clamp
            nanq[g, :, :, t, :] = np.isnan(sl)
            codes[g, :, :, t, :] = np.where(np.isnan(sl), F32(0), r).astype(np.int8)
    if nan_as_qmin:
        codes = np.where(nanq, np.int8(QMIN[kind]), codes)
    if kind == "int4":
        q = O.pack_int4(codes)
        if nibble_zero:
            if D % 2:
                nanq = np.concatenate([nanq, np.zeros_like(nanq[..., :1])], axis=-1)
            q = q & np.where(nanq[..., 0::2], np.uint8(0x0F), np.uint8(0xFF)) & np.where(nanq[..., 1::2], np.uint8(0xF0), np.uint8(0xFF))
    else:
        q = codes
    stored = O.stored_scale_as_f32(O._round_to_storage(s32, case.x, odt(case.dtype)), odt(case.dtype))
    return q, stored


def contract_absmax(x: np.ndarray, dtype: str, table: np.ndarray | None = None, *, forget_nan=False, drop_nan=False):
    """[G, T] abs-max table by the contract: NaN for a slice with a NaN, else +inf for one with an inf; ``table``: the
    accumulating entry point, which keeps a NaN the table already holds. forget_nan: it takes fmaxf(old, new) instead."""
    x32 = widen(x, dtype)
    a = np.abs(x32)
    am = (np.fmax.reduce(a, axis=(1, 2, 4)) if drop_nan else a.max(axis=(1, 2, 4))).astype(F32)
    if table is None:
        return am
    return (np.fmax(table, am) if forget_nan else np.maximum(table, am)).astype(F32)


def quant_cases(shape, dtype: str, kind: str, given_table: bool, max_chunks: int = 2) -> list:
    """Every family for one route: the data-maximum families, and the table family for the from_absmax entry point
    (there the other families pass the data's own maximum as the table)."""
    out = exhaustive_cases(shape, dtype, kind, max_chunks) + tie_cases(shape, dtype, kind) + probe_cases(shape, dtype) + \
        eps_cases(shape, dtype)
    if given_table:
        out += table_cases(shape, dtype)
    return out


def reference(case: Case, kind: str):
    """The oracle's (q, scales_f32) for a case: the data's own abs-max, or the case's table."""
    if case.table is None:
        q, _, s = O.quantize_tokens(case.x, kind, case.eps, odt(case.dtype))
    else:
        q, _, s = O.quantize_tokens_with_absmax(case.x, case.table, kind, case.eps, odt(case.dtype))
    return q, s


# ------------------------------------------------------------------------------------------- exact emulation

def _sig(v32: np.ndarray):
    """fp32 values as (int64 m, int64 e) with v = m * 2^e exactly"""
    m, e = np.frexp(np.asarray(v32, dtype=np.float64))
    return (m * 2.0 ** 24).astype(np.int64), e.astype(np.int64) - 24


def _rint_exact(m: np.ndarray, e: np.ndarray, away: bool):
    """(k, d): k = the integer nearest m * 2^e (ties to even, or away from zero), d = m * 2^e - k as float64 (exact).
    Integer arithmetic on the significands: valid for |m * 2^e| < 2^62."""
    k = np.zeros_like(m)
    d = np.zeros(m.shape, dtype=np.float64)
    pos = e >= 0
    k[pos] = m[pos] << e[pos]
    neg = ~pos & (-e <= 60)
    sh = -e[neg]
    mm = m[neg]
    q = mm >> sh                      # floor
    rem = mm - (q << sh)              # in [0, 2^sh)
    half = np.int64(1) << (sh - 1)
    up = (rem > half) | ((rem == half) & ((mm > 0) if away else (q & 1) == 1))
    kk = q + up
    k[neg] = kk
    d[neg] = np.ldexp((mm - (kk << sh)).astype(np.float64), -sh)
    tiny = ~pos & (-e > 60)           # |value| < 2^-12: rounds to 0
    d[tiny] = np.ldexp(m[tiny].astype(np.float64), e[tiny])
    return k, d


def emulate_quotient(x32: np.ndarray, s32: np.ndarray, kind: str, *, fallback=True, clamp=True, fused=True,
                     away=False) -> np.ndarray:
    """The magic sums of ``quotient_bits8`` as uint32 fp32 bit patterns, for x32 [..., D] (D % 8 == 0) and s32
    broadcastable to it. Exact: ``x * r`` is formed from the integer significands (48 bits), its nearest integer by
    integer shifts, and the fp32 sum ``RN(x*r + magic)`` equals ``magic + rint(x*r)`` while |x*r| < 2^22; past that the
    sum of the 48-bit product and the magic number spans at most 50 bits, which a float64 holds exactly before the
    one rounding to fp32.
      fallback=False  never redo a vector with the IEEE division
      clamp=False     no clamp of the sum or of the redo (what the vector kernels did before the from_absmax fix)
      fused=False     round RN(x * RN(1/s32)) (two roundings) and never redo: the quotient without its guard
      away=True       round half away from zero instead of half to even"""
    x32 = np.asarray(x32, dtype=F32)
    s32 = np.broadcast_to(np.asarray(s32, dtype=F32), x32.shape)
    bias = 0 if kind == "int8" else 8
    magic = F32(12582912.0 + bias)
    lo, hi = F32(float(magic) + QMIN[kind]), F32(float(magic) + QMAX[kind])
    km = F32(1.5) * F32(QMAX[kind]) * F32(2.0 ** -22)
    thr = F32(0.5) - km
    r = (F32(1) / s32).astype(F32)
    if not fused:
        p = (x32 * r).astype(F32)
        k, _ = _rint_exact(*_sig(p), away)
        sums = (k.astype(np.float64) + float(magic)).astype(F32)
        if clamp:
            sums = np.clip(sums, lo, hi)
        return sums.view(np.uint32)
    mx, ex = _sig(x32)
    mr, er = _sig(r)
    m, e = mx * mr, ex + er                      # x * r exactly
    p64 = np.ldexp(m.astype(np.float64), e)      # exact: 48 significant bits
    small = np.abs(p64) < 2.0 ** 22
    k, d_small = _rint_exact(np.where(small, m, 0), np.where(small, e, 0), away)
    with np.errstate(over="ignore", invalid="ignore"):
        sums_big = (p64 + float(magic)).astype(F32)
        t = (magic - sums_big).astype(F32)
        d_big = (p64 + t.astype(np.float64)).astype(F32)
    sums = np.where(small, (k.astype(np.float64) + float(magic)).astype(F32), sums_big)
    d = np.where(small, d_small.astype(F32), d_big)
    if clamp:
        sums = np.clip(sums, lo, hi)
    if fallback:
        shp = x32.shape[:-1] + (x32.shape[-1] // 8, 8)
        worst = np.fmax.reduce(np.abs(d).reshape(shp), axis=-1)   # fmaxf: a NaN does not count
        redo = np.repeat(worst >= thr, 8, axis=-1).reshape(x32.shape)
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            y = (x32 / s32).astype(F32)                            # IEEE fp32 division
            if away:
                qf = (np.sign(y) * np.floor(np.abs(y).astype(np.float64) + 0.5)).astype(F32)
            else:
                qf = np.rint(y).astype(F32)
        if clamp:
            qf = np.clip(qf, F32(QMIN[kind]), F32(QMAX[kind]))
        with np.errstate(over="ignore", invalid="ignore"):
            sums = np.where(redo, (qf + magic).astype(F32), sums)
    return np.asarray(sums, dtype=F32).view(np.uint32)


def pack_bytes(sums: np.ndarray, kind: str) -> np.ndarray:
    """``pack_i8`` / ``pack_i4`` of magic sums [..., D]: the low byte of each sum; INT4 pairs as
    ((n_even << 4) | n_odd) & 0xFF, so an odd element's byte above 15 spills into the even element's nibble."""
    b = (sums & np.uint32(0xFF)).astype(np.uint32)
    if kind == "int8":
        return b.astype(np.uint8).view(np.int8)
    return (((b[..., 0::2] << np.uint32(4)) | b[..., 1::2]) & np.uint32(0xFF)).astype(np.uint8)


def emulate_quant(case: Case, kind: str, **switches):
    """(q, scales_f32) of a vector quantise route for ``case`` under the emulation (D % 8 == 0)."""
    x32 = widen(case.x, case.dtype)
    am = data_absmax(case.x, case.dtype) if case.table is None else case.table
    s32 = scale32(am, kind, case.eps)                       # [G, T]
    sums = emulate_quotient(x32, s32[:, None, None, :, None], kind, **switches)
    stored = O.stored_scale_as_f32(O._round_to_storage(s32, case.x, odt(case.dtype)), odt(case.dtype))
    return pack_bytes(sums, kind), stored


# ------------------------------------------------------------------------------------------------ case statistics

def stats(case: Case, kind: str) -> dict:
    """How often a case reaches each edge: exact ties x/s32 = k + 1/2, 8-element vectors that take the division redo,
    tokens on the eps floor, elements the reference's clamp changes."""
    x32 = widen(case.x, case.dtype).astype(np.float64)
    am = data_absmax(case.x, case.dtype) if case.table is None else case.table
    s32 = scale32(am, kind, case.eps)
    s = s32[:, None, None, :, None].astype(np.float64)
    k2 = np.rint(2 * x32 / s)
    ties = int(((k2 % 2 == 1) & (k2 * s == 2 * x32)).sum())
    d = case.x.shape[-1]
    guard = 0
    if d % 8 == 0:  # 8-element vectors whose product x * RN(1/s32) (exact in float64) is within kM of a half-integer
        km = F32(1.5) * F32(QMAX[kind]) * F32(2.0 ** -22)
        r = (F32(1) / s32).astype(F32)[:, None, None, :, None]
        p = x32 * r.astype(np.float64)
        dd = np.abs(p - np.rint(p))
        guard = int((dd.reshape(dd.shape[:-1] + (d // 8, 8)).max(-1) >= 0.5 - float(km)).sum())
    with np.errstate(over="ignore", invalid="ignore"):
        q = np.rint((widen(case.x, case.dtype) / s32[:, None, None, :, None]).astype(F32))
    clamps = int(((q > QMAX[kind]) | (q < QMIN[kind])).sum())
    eps_floor = int((am.astype(F32) / F32(QMAX[kind]) < F32(case.eps)).sum())
    return {"ties": ties, "guard": guard, "eps_floor": eps_floor, "clamp": clamps}


# ------------------------------------------------------------------------------------------------ dequantise codes

def dequant_code_cases(kind: str, out_dtype: str, T: int = 9, H: int = 2, D: int = 512):
    """(name, q [1,1,H,T,Dq], scales_f32 [1,T]): every byte value (INT8: all 256 codes incl. -128; INT4: all 256
    packed bytes, i.e. every nibble pair) in every token, against per-token scales whose products are fp16 / bf16
    subnormals, overflow fp16 to inf, are exact ties of the output dtype, or a stored scale of +0 / -0; and a second
    case with the scales NaN, +inf and -inf (compare with :func:`float_mismatch`)."""
    Dq = D if kind == "int8" else D // 2
    codes = np.arange(256, dtype=np.uint32).astype(np.uint8)
    row = np.resize(codes, Dq)
    q = np.broadcast_to(row, (1, 1, H, T, Dq)).copy()
    q[0, 0, 1] = np.roll(row, 37)                       # the second head: the codes in another order
    if kind == "int8":
        q = q.view(np.int8)
    # 1 + half an fp16 ulp: q * tie16 is exactly halfway between two fp16 values for q = ±1, ±2, ±4, ... (the
    # power-of-two codes; 3 * tie16 is 0.75 ulp past 3, not a tie). tieb does the same for bf16.
    tie16 = F32(1 + 2.0 ** -11)
    tieb = F32(1 + 2.0 ** -8)
    sc = np.array([2.0 ** -24, 2.0 ** -20,            # fp16 subnormal products
                   2.0 ** -133, 1e-39,                # bf16 / fp32 subnormal products
                   1024.0, 3.0e36,                    # fp16 overflow to inf (and bf16 near its top)
                   tie16 if out_dtype != "bf16" else tieb, -0.0, 0.0], dtype=F32)
    scales = np.resize(sc, T).astype(F32)[None, :]
    # what a poisoned token stores: the products are NaN (any scale NaN; code 0 times inf) or ±inf
    bad = np.resize(np.array([np.nan, np.inf, -np.inf], dtype=F32), T).astype(F32)[None, :]
    return [("codes_x_scales", q, scales), ("codes_x_nonfinite_scales", q, bad)]
