"""Far layouts: tiny logical tensors spread over one large arena, so that the ADDRESSES a kernel computes are those of the
full-size workload and beyond (Llama-3-8B at batch 64 and 32 K tokens: the last batch rows of one launch start more than
2^31 bytes, for the fp16 side more than 2^32 bytes, from the pointer the kernel was given) while the WORK stays a few
hundred KB. Host arithmetic only (no torch, no GPU): tests/test_far_layouts_host.py checks every layout of :data:`TABLE` on the CPU,
tests/test_far_offsets_discrimination.py shows that the checks reject 32-bit addressing, tests/test_gpu_far_offsets.py runs
the kernels on them.

One arena is a single uint8 allocation of :data:`ARENA_BYTES`, every byte :data:`FILL` (0x5A: INT8 code 90, INT4 nibbles
5 / 10, fp16 203.25, an fp32 scale of 1.5e16, an int32 far out of range as a gather index). A :class:`FarTensor` is a
base offset into it, byte strides for every dim but the last (contiguous) one, a logical shape and a dtype; a
:class:`Layout` is the tensors of one call. Dims whose byte stride is at least :data:`OUTER` are the tensor's FAR dims;
the rest (tokens, mostly) span a small contiguous BLOCK behind every far index tuple.

What :func:`far_report`, :func:`alignment_faults` and :func:`safety_faults` check, per tensor and per layout:

* some block starts more than 2^31 bytes from the tensor's base and some more than 2^32; some single ``index * stride``
  product exceeds 2^31 and some 2^32; for 2- and 4-byte tensors (whose strides the ABI takes in elements) some block's
  ELEMENT offset exceeds 2^31 as well;
* every stride is a multiple of 16 bytes (so of 8 fp16 elements), every base 16-byte aligned: the fast routes stay open;
* every address a plausibly wrong kernel could compute — any subset of the products, or their sum, truncated to int32
  (sign-extended) or uint32, or a stride truncated before the multiply, in byte or in element arithmetic
  (:func:`wrong_starts`) — lies inside the arena and on no true block of any tensor of the layout. A narrowing bug then
  reads 0x5A or writes onto it: a wrong answer or a dirty arena, never a fault.

An fp32 tensor whose element offset passes 2^31 sits more than 8 GiB from its base, and an int32 element offset wraps it
down by 16 GiB: its far blocks must lie above 16 GiB, which sets the arena's size (17.5 GiB) and the fp32 tensors' base.
"""
import itertools
from bisect import bisect_right

FILL = 0x5A
KiB, MiB, GiB = 1 << 10, 1 << 20, 1 << 30
ARENA_BYTES = 35 * GiB // 2
OUTER = 1 << 20
ESZ = {"i8": 1, "u8": 1, "f16": 2, "bf16": 2, "f32": 4}
CODES = {"int8": "i8", "int4": "u8"}
P1 = (1 << 32) + (1 << 28)   # base of 1- and 2-byte far tensors: two negative int32 wraps of byte products stay inside
P4 = (1 << 33) + (1 << 28)   # base of fp32 far tensors: one negative int32 wrap of an ELEMENT offset (up to 2^33 bytes)
SLOT = (1 << 25) + 3 * (1 << 18)  # the tensors of one call are shifted by multiples of this (blocks are tiny against it)


def packed(kind, D):
    return D if kind == "int8" else (D + 1) // 2


class FarTensor:
    """``shape`` logical, ``strides`` in BYTES for every dim but the last (which is contiguous), ``base`` the byte offset of
    element 0 in the arena. ``far=False``: a guard-boundary tensor (its offsets stay below 2^31 on purpose); it must be safe
    and aligned, not far."""

    def __init__(self, name, dtype, base, shape, strides, far=True, odd_rows=False):
        assert len(strides) == len(shape) - 1, (name, shape, strides)
        self.name, self.dtype, self.base, self.shape, self.strides, self.far = name, dtype, int(base), tuple(shape), tuple(strides), far
        self.odd_rows = odd_rows  # a row length picked to close the fast routes: only the far strides must be aligned
        self.esz = ESZ[dtype]
        self.row_bytes = self.shape[-1] * self.esz
        self.outer = [i for i, s in enumerate(self.strides) if s >= OUTER and self.shape[i] > 1]
        self.inner = [i for i in range(len(self.strides)) if i not in self.outer]
        self.block_bytes = sum((self.shape[i] - 1) * self.strides[i] for i in self.inner) + self.row_bytes
        self.extent = sum((n - 1) * s for n, s in zip(self.shape, self.strides)) + self.row_bytes

    def elem_strides(self):
        """what ``as_strided`` and the ABI take: element strides of every dim (the last one 1)"""
        assert all(s % self.esz == 0 for s in self.strides), self.name
        return tuple(s // self.esz for s in self.strides) + (1,)

    def outer_indices(self):
        return itertools.product(*(range(self.shape[i]) for i in self.outer))

    def products(self, idx):
        return [j * self.strides[i] for i, j in zip(self.outer, idx)]

    def blocks(self):
        """{far index tuple: byte offset of its block in the arena}"""
        return {idx: self.base + sum(self.products(idx)) for idx in self.outer_indices()}

    def rows(self):
        """byte offset in the arena of every logical row (every index tuple over all dims but the last)"""
        for idx in itertools.product(*(range(n) for n in self.shape[:-1])):
            yield idx, self.base + sum(j * s for j, s in zip(idx, self.strides))

    def __repr__(self):
        return f"FarTensor({self.name}, {self.dtype}, base={self.base:#x}, shape={self.shape}, strides={self.strides})"


class Layout:
    def __init__(self, name, tensors, arena=ARENA_BYTES):
        self.name, self.arena = name, arena
        self.t = {t.name: t for t in tensors}
        assert len(self.t) == len(tensors), name

    def __getitem__(self, key):
        return self.t[key]


def trunc(v, how):
    """``v`` kept in 32 bits: ``i32`` two's complement with sign extension, ``u32`` zero extension"""
    v &= 0xFFFFFFFF
    return v - (1 << 32) if (how == "i32" and v >= 1 << 31) else v


def far_report(t):
    """The far requirements of the module docstring for one tensor, each a bool."""
    offs = [o - t.base for o in t.blocks().values()]
    prods = [p for idx in t.outer_indices() for p in t.products(idx)]
    return dict(row31=any(o > 1 << 31 for o in offs), row32=any(o > 1 << 32 for o in offs),
                prod31=any(p > 1 << 31 for p in prods), prod32=any(p > 1 << 32 for p in prods),
                elem31=t.esz == 1 or any(o // t.esz > 1 << 31 for o in offs))


def alignment_faults(t):
    """strides and base that would close a fast route: not multiples of 16 bytes (8 elements of a 2-byte type)"""
    bad = [f"{t.name}: stride {s} of dim {i}" for i, s in enumerate(t.strides)
           if s % t.esz or (s % 16 and not (t.odd_rows and i in t.inner))]
    return bad + ([f"{t.name}: base {t.base}"] if t.base % 16 else [])


def wrong_starts(t):
    """{wrong block start in the arena: what computed it} over every far index tuple of ``t``: any non-empty subset of the
    products truncated, the sum truncated, or the subset's strides truncated before the multiply; int32 and uint32; in byte
    arithmetic and, for 2- and 4-byte tensors, in element arithmetic (scaled to bytes afterwards). Results equal to the
    tuple's true start are left out."""
    out = {}
    n = len(t.outer)
    subsets = [s for r in range(1, n + 1) for s in itertools.combinations(range(n), r)]
    for idx in t.outer_indices():
        prods = t.products(idx)
        true = t.base + sum(prods)
        for unit in {1, t.esz}:
            p = [x // unit for x in prods]
            st = [t.strides[i] // unit for i in t.outer]
            for how in ("i32", "u32"):
                cands = [("sum", trunc(sum(p), how))]
                for s in subsets:
                    cands.append((f"products {s}", sum(trunc(x, how) if k in s else x for k, x in enumerate(p))))
                    cands.append((f"strides {s}", sum(j * trunc(st[k], how) if k in s else p[k] for k, j in enumerate(idx))))
                for what, off in cands:
                    a = t.base + off * unit
                    if a != true:
                        out.setdefault(a, f"{t.name}{idx}: {what} as {how}, unit {unit}")
    return out


def safety_faults(layout):
    """Wrong block starts (:func:`wrong_starts`) of every tensor of ``layout`` that leave the arena or touch a true block of
    any tensor; true blocks that leave the arena or overlap each other. Empty when the layout is safe."""
    true = sorted((start, start + t.block_bytes, t.name) for t in layout.t.values() for start in t.blocks().values())
    bad = []
    for (a0, a1, na), (b0, b1, nb) in zip(true, true[1:]):
        if b0 < a1:
            bad.append(f"true blocks of {na} and {nb} overlap at {b0:#x}")
    if true and (true[0][0] < 0 or true[-1][1] > layout.arena):
        bad.append("a true block lies outside the arena")
    starts = [x[0] for x in true]
    for t in layout.t.values():
        for w, what in wrong_starts(t).items():
            if w < 0 or w + t.block_bytes > layout.arena:
                bad.append(f"{what}: {w:#x} outside the arena")
                continue
            k = bisect_right(starts, w + t.block_bytes - 1)  # true blocks that start before the wrong block's end
            if k and true[k - 1][1] > w:
                bad.append(f"{what}: {w:#x} on a true block of {true[k - 1][2]}")
    return bad


# ----------------------------------------------------------------------------------------------------- addressing models
# How a kernel may turn a far index tuple into a block offset. "exact" is what the library must do; every other model
# is one narrowing mistake (tests/test_far_offsets_discrimination.py runs them against the checks of the GPU test).
MODELS = ("exact", "sum_i32", "sum_u32", "product_i32", "product_u32", "stride_i32", "stride_u32", "elem_i32", "elem_u32")


def block_start(t, idx, model="exact"):
    """Arena byte offset of the block behind far index tuple ``idx`` of ``t`` as ``model`` computes it.
    sum_*: the byte offset's sum kept in 32 bits; product_*: every ``index * stride`` product; stride_*: every stride
    narrowed before the multiply; elem_*: the ELEMENT offset kept in 32 bits, then scaled to bytes in 64."""
    prods = t.products(idx)
    if model == "exact":
        return t.base + sum(prods)
    kind, how = model.split("_")
    if kind == "sum":
        return t.base + trunc(sum(prods), how)
    if kind == "product":
        return t.base + sum(trunc(p, how) for p in prods)
    if kind == "stride":
        return t.base + sum(j * trunc(t.strides[i], how) for i, j in zip(t.outer, idx))
    assert kind == "elem", model
    return t.base + trunc(sum(prods) // t.esz, how) * t.esz


def moved(t, model):
    """far index tuples of ``t`` whose block ``model`` puts somewhere else"""
    return [idx for idx in t.outer_indices() if block_start(t, idx, model) != block_start(t, idx)]


# ------------------------------------------------------------------------------------------------------- stride families
# [G, B, H] = [2, 3, 2]; batch and head strides independent (the 5-D entry points' strided kernels)
FIVE = ((1 << 32) + (1 << 26), (1 << 30) + (1 << 24), 3 << 29)
# the fp32 form: the group stride alone passes 2^31 ELEMENTS (see the module docstring), batch and head strides stay small
FIVE_F32 = ((1 << 33) + (1 << 27), (1 << 28) + (1 << 22), (1 << 27) + (1 << 19))
# behind a FIVE tensor (which ends below 12 GiB): the group stride alone is far
FIVE_BEHIND = ((1 << 32) + (1 << 26), (1 << 28) + (1 << 22), (1 << 27) + (1 << 19))
# the same with batch rows contiguous over heads (b = H * h): what Wave / Block256 / Tile ask of both sides
ROWS_H = (1 << 29) + (1 << 22)
ROWS = ((1 << 32) + (1 << 26), 2 * ROWS_H, ROWS_H)
# [G, B, H] = [2, 33, 4]: more than 16,384 elements per token (Wide, Sweep at a power-of-two head_dim)
MANY = ((1 << 32) + (1 << 26), (1 << 26) + (1 << 19), (1 << 23) + (1 << 16))
# [G, B, H] = [2, 1, 8] and [2, 17, 8], batch rows contiguous over heads and every group's rows within 2 GiB: what the one-wave
# tile kernels ask (their spans are guarded, tests/test_gpu_far_offsets.py runs the guards too); the GROUP stride is the far one
TILE_H = (1 << 24) + 5 * (1 << 14)
TILE = ((1 << 32) + (1 << 26), 8 * TILE_H, TILE_H)
WALK_H = (1 << 23) + 7 * (1 << 12)
WALK = ((1 << 32) + (1 << 26), 8 * WALK_H, WALK_H)
# one layer's store [B, Hkv <= 8] with B = 2, and [B, Hq, D] / [B, Hkv, D] rows beside it
ATTN = ((1 << 32) + (1 << 26), (1 << 29) + (1 << 20))
SCALES_G = (1 << 33) + (1 << 27)  # [G, T] fp32 tables: more than 2^31 floats between the groups' rows
MASS_B = (1 << 33) + (1 << 27)    # key_scores' fp32 [B, Hkv, T]: batch rows more than 2^31 floats apart
TOKEN_FAR = (1 << 24) + (1 << 12)  # a far TOKEN stride: batch rows and heads interleaved inside it


def base_of(dtype, slot):
    return (P4 if ESZ[dtype] == 4 else P1) + slot * SLOT


def five(name, dtype, slot, T, D, family=FIVE, gbh=(2, 3, 2)):
    """[G, B, H, T, D] with token rows contiguous"""
    if dtype == "f32" and family is FIVE:
        family = FIVE_F32
    return FarTensor(name, dtype, base_of(dtype, slot), gbh + (T, D), family + (D * ESZ[dtype],), odd_rows=D * ESZ[dtype] % 16 != 0)


def scales(name, slot, G, T):
    return FarTensor(name, "f32", base_of("f32", slot), (G, T), (SCALES_G,))


def quant_layout(name, dtype, kind, T, D, family=FIVE, gbh=(2, 3, 2)):
    """kvq_quant_*_tokens / kvq_absmax_tokens / kvq_quant_tokens_from_absmax: x, the store window q, the scale rows"""
    return Layout(name, [five("x", dtype, 0, T, D, family, gbh), five("q", CODES[kind], 1, T, packed(kind, D), family, gbh),
                         scales("scales", 2, gbh[0], T)])


def dequant_layout(name, kind, out_dtype, T, D, t_pad=0):
    """kvq_dequant_*_tokens; ``t_pad`` > 0: token rows of the output ``t_pad`` elements apart more than D (Generic route)"""
    out = five("out", out_dtype, 1, T, D)
    if t_pad:
        out = FarTensor("out", out_dtype, out.base, out.shape, out.strides[:3] + ((D + t_pad) * ESZ[out_dtype],))
    return Layout(name, [five("q", CODES[kind], 0, T, packed(kind, D)), out, scales("scales", 2, 2, T)])


def evict_layout(name, dtype, T, Tout, D):
    """kvq_window_compact / kvq_gather_tokens / kvq_chunk_meanpool: x [G,B,H,T,D] -> out [G,B,H,Tout,D]"""
    return Layout(name, [five("x", dtype, 0, T, D), five("out", dtype, 1, Tout, D)])


def store_pool_layout(name, kind, T, Tout, D, far_scales):
    """kvq_store_chunk_pool: codes and scale rows of the store going in and of the one coming out. The entry point refuses
    an output whose extent (base to last byte) meets the input's, so the two far code tensors follow each other (the
    output on the shorter FIVE_BEHIND strides), and only one of the two scale tables (``far_scales``: "in" / "out") can
    have its rows more than 2^31 floats apart; the other is a plain contiguous table below the far bases."""
    dq = packed(kind, D)
    q_in = five("q_in", CODES[kind], 0, T, dq)
    q_out = FarTensor("q_out", CODES[kind], 12 * GiB + SLOT, (2, 3, 2, Tout, dq), FIVE_BEHIND + (dq,), odd_rows=dq % 16 != 0)
    assert q_in.base + q_in.extent <= q_out.base
    n = {"in": T, "out": Tout}
    near = "out" if far_scales == "in" else "in"
    return Layout(name, [q_in, q_out, scales("s_" + far_scales, 2, 2, n[far_scales]),
                         FarTensor("s_" + near, "f32", (1 << 27) + SLOT, (2, n[near]), (-(-n[near] // 4) * 16,), far=False)])


def attn_layout(name, B, Hq, Hkv, cap, D, kinds, S=0, layers=0):
    """One layer's decode (S = 0) or extend (S query tokens) call: K / V code stores [B,Hkv,cap,Dq], q / out [B,Hq,(S,)D],
    k_new / v_new [B,Hkv,(S,)D] (fp16 and bf16 share the layout: 2 bytes). ``layers`` = L > 0: the [L, ...] tensors of
    kvq_decode_step_layers, the layers' stores more than 2^32 bytes apart, their scale rows [L, cap] as well."""
    sb, sh = ATTN
    lead, ls = ((layers,), ((1 << 32) + (1 << 27),)) if layers else ((), ())
    sb2 = (1 << 31) + (1 << 25) if layers else sb  # 2-byte tensors: one dim alone may pass 2^31 elements (two wraps stack)
    mid, ms = ((S,), (D * 2,)) if S else ((), ())
    hq = (S or 1) * D * 2
    tens = []
    for i, (n, kind) in enumerate(zip("kv", kinds)):
        dq = packed(kind, D)
        tens.append(FarTensor(n + "_store", CODES[kind], base_of("u8", i), lead + (B, Hkv, cap, dq), ls + (sb, sh, dq)))
    for i, n in enumerate(("q", "out")):
        tens.append(FarTensor(n, "f16", base_of("f16", 2 + i), lead + (B, Hq) + mid + (D,), ls + (sb2, hq) + ms))
    for i, n in enumerate(("k_new", "v_new")):
        tens.append(FarTensor(n, "f16", base_of("f16", 4 + i), lead + (B, Hkv) + mid + (D,), ls + (sb2, sh) + ms))
    if layers:
        tens += [scales("k_scales", 6, layers, cap), scales("v_scales", 7, layers, cap)]
    return Layout(name, tens)


def key_scores_layout(name, B, Hq, Hkv, T, S, D, kind, far_tokens=False):
    """kvq_key_scores: q [B,Hq,S,D], the K store, mass fp32 [B,Hkv,T]. ``far_tokens``: the store's TOKEN stride is the far
    one (batch rows and heads interleaved inside it)."""
    sb, sh = ATTN
    dq = packed(kind, D)
    kst = (Hkv * 4 * KiB, 4 * KiB, TOKEN_FAR) if far_tokens else (sb, sh, dq)
    return Layout(name, [FarTensor("k_store", CODES[kind], base_of("u8", 0), (B, Hkv, T, dq), kst),
                         FarTensor("q", "f16", base_of("f16", 2), (B, Hq, S, D), (sb, S * D * 2, D * 2)),
                         FarTensor("mass", "f32", base_of("f32", 3), (B, Hkv, T), (MASS_B, sh))])


# ------------------------------------------------------------------------------------------------------ guard boundaries
LIMIT = 1 << 31


def under_and_at(limit, count, fixed=0, align=16):
    """The largest stride s (a multiple of ``align``) with ``count * s + fixed < limit`` and the smallest with
    ``count * s + fixed >= limit``: the two sides of a host guard of that form."""
    under = (limit - 1 - fixed) // count // align * align
    at = -(-(limit - fixed) // count) + align - 1
    at = at // align * align
    assert count * under + fixed < limit <= count * at + fixed and at - under <= align, (limit, count, fixed)
    return under, at


TILE_SHAPE = (1, 1, 8, 8, 128)  # quant_tile_k<., ., 8, 16, 4>: R = 8 rows, tt = 4 tokens per tile
SPLIT_SHAPE = (1, 17, 8, 8, 128)  # the Split walk: R = 136 rows, more than 16,384 elements per token


def tile_guard(kind):
    """quant_route's Tile guard: span_in = (R - 1) * is.h * 2 + tt * D * 2 and span_q = (R - 1) * qs.h + tt * Dq, both below
    2^31. -> {"in": (under, at), "q": (under, at)} head strides in BYTES."""
    G, B, H, T, D = TILE_SHAPE
    return {"in": under_and_at(LIMIT, B * H - 1, 4 * D * 2), "q": under_and_at(LIMIT, B * H - 1, 4 * packed(kind, D))}


def split_guard():
    """split_walk_ok's guards: (R - 1) * is.h * 2 + 8 * D * 2 and (R - 1) * qs.h + 8 * D, both below 2^31"""
    G, B, H, T, D = SPLIT_SHAPE
    return {"in": under_and_at(LIMIT, B * H - 1, 8 * D * 2), "q": under_and_at(LIMIT, B * H - 1, 8 * D)}


def guard_quant_layout(name, shape, kind, in_h, q_h):
    """x and q of one quantise call with the given head strides (bytes), batch rows contiguous over heads, one group"""
    G, B, H, T, D = shape
    dq = packed(kind, D)
    x = FarTensor("x", "f16", 1 << 28, shape, (0, H * in_h, in_h, D * 2), far=False)
    q = FarTensor("q", CODES[kind], (1 << 28) + (5 << 29) + (1 << 22), (G, B, H, T, dq), (0, H * q_h, q_h, dq), far=False)
    s = FarTensor("scales", "f32", 1 << 27, (G, T), (T * 4,), far=False)
    return Layout(name, [x, q, s])


POOL_GUARD = dict(D=128, chunk=32, n_full=1, ragged=3, keep=2)  # chunk_pool_wave_k<., 4, 8>; T = 37: below 2^32 bytes


def pool_guard():
    """pool_route's Wave guard: chunk_size * isb.t below 2^31 -> (under, at) token strides in bytes"""
    return under_and_at(LIMIT, POOL_GUARD["chunk"])


def guard_pool_layout(name, dtype, t_stride):
    g = POOL_GUARD
    T = g["chunk"] * g["n_full"] + g["ragged"] + g["keep"]
    x = FarTensor("x", dtype, (1 << 31) + (1 << 28), (1, 1, 2, T, g["D"]), (0, 0, 64 * KiB, t_stride), far=False)
    out = FarTensor("out", dtype, (1 << 27) + (1 << 20), (1, 1, 2, g["n_full"] + 1 + g["keep"], g["D"]), (0, 0, 4 * KiB, g["D"] * 2), far=False)
    return Layout(name, [x, out])


ROW_GUARD_T = 600  # stored tokens of the decode row-limit cases


def row_guard():
    """decode_attn_impl's row limit: T * st.t below 2^31 -> (under, at) token strides in bytes"""
    return under_and_at(LIMIT, ROW_GUARD_T)


def guard_attn_layout(name, Hq, D, kinds, t_stride):
    """B = 1, Hkv = 1, a padded token stride: K and V are 2 GiB of arena each, T * Dq bytes of each are touched"""
    T = ROW_GUARD_T
    tens = [FarTensor(n + "_store", CODES[kind], (1 << 31) + (1 << 28) + i * ((1 << 31) + (1 << 27)), (1, 1, T + 1, packed(kind, D)), (0, 0, t_stride), far=False)
            for i, (n, kind) in enumerate(zip("kv", kinds))]
    return Layout(name, tens)


# ---------------------------------------------------------------------------------------------------------------- table
def _table():
    tab = []
    for kind in ("int8", "int4"):
        k = kind[3:]
        # quantise: Generic (independent batch / head strides and fp32, or an odd head_dim), Sweep (D = 96), Wave and
        # Block256 (batch rows contiguous over heads), Wide and Sweep at D = 128 (132 rows)
        tab += [quant_layout(f"quant{k}_f32_generic", "f32", kind, 5, 128),
                quant_layout(f"quant{k}_odd_generic", "f16", kind, 5, 20),
                quant_layout(f"quant{k}_sweep96", "bf16", kind, 5, 96),
                quant_layout(f"quant{k}_wave", "f16", kind, 9, 128, ROWS),
                quant_layout(f"quant{k}_blk256", "bf16", kind, 3, 128, ROWS),
                quant_layout(f"quant{k}_many", "f16", kind, 5, 128, MANY, (2, 33, 4)),
                quant_layout(f"quant{k}_tile", "f16", kind, 9, 128, TILE, (2, 1, 8)),
                quant_layout(f"quant{k}_split", "bf16", kind, 5, 128, WALK, (2, 17, 8))]
        tab += [dequant_layout(f"dequant{k}_{dt}", kind, dt, 37, 128) for dt in ("f16", "bf16", "f32")]
        tab += [dequant_layout(f"dequant{k}_generic", kind, "f16", 5, 64, t_pad=8)]
        for far_scales in ("in", "out"):
            tab += [store_pool_layout(f"store_pool{k}_fast_{far_scales}", kind, 16 * 2 + 3 + 4, 2 + 1 + 4, 64, far_scales),
                    store_pool_layout(f"store_pool{k}_generic_{far_scales}", kind, 7 * 2 + 3 + 4, 2 + 1 + 4, 24, far_scales)]
    for dt in ("f16", "bf16", "f32"):
        tab += [evict_layout(f"evict_{dt}", dt, 32 * 2 + 3 + 4, 7, 128),    # window 7 / gather 7 / pool: chunk 32, keep 4
                evict_layout(f"evict_{dt}_d20", dt, 7 * 2 + 3 + 4, 7, 20)]  # 40-byte rows: Scalar copies, Generic pool
    tab += [evict_layout("evict_f16_vec", "f16", 7 * 2 + 3 + 4, 7, 192)]  # 24 vectors per row: gather Vec, pool Vec
    from tests.attn_cases import DECODE_ROUTES, EXTEND_ROUTES, KINDS
    for route, ((B, Hq, Hkv, T, D), _, _, _) in DECODE_ROUTES.items():
        tab.append(attn_layout("decode " + route, B, Hq, Hkv, T + 3, D, KINDS))
    B, Hq, Hkv, T, D = DECODE_ROUTES["ring hd128 TG4"][0]
    tab.append(attn_layout("decode layers", B, Hq, Hkv, T + 3, D, KINDS, layers=2))
    for route in ("one split", "splits + merge"):
        (_, Hq, Hkv, T, S, D), _ = EXTEND_ROUTES[route]
        tab.append(attn_layout("extend " + route, 2, Hq, Hkv, T, D, KINDS, S=S))
    for kind in ("int8", "int4"):
        tab += [key_scores_layout(f"key_scores {kind}", 2, 8, 2, 319, 16, 128, kind),
                key_scores_layout(f"key_scores {kind} far tokens", 2, 8, 2, 319, 16, 128, kind, far_tokens=True)]
    # guard boundaries: the largest admissible stride under each bound and the smallest at it
    for kind in ("int8", "int4"):
        tg, sg = tile_guard(kind), split_guard()
        for side, (i, q) in (("under", (0, 0)), ("in_at", (1, 0)), ("q_at", (0, 1))):
            tab += [guard_quant_layout(f"guard tile {kind} {side}", TILE_SHAPE, kind, tg["in"][i], tg["q"][q]),
                    guard_quant_layout(f"guard split {kind} {side}", SPLIT_SHAPE, kind, sg["in"][i], sg["q"][q])]
    for dt in ("f16", "bf16"):
        tab += [guard_pool_layout(f"guard pool {dt} {side}", dt, pool_guard()[i]) for i, side in enumerate(("under", "at"))]
    tab += [guard_attn_layout(f"guard rows {side}", 4, 128, KINDS, row_guard()[i]) for i, side in enumerate(("under", "at"))]
    return tab


TABLE = {l.name: l for l in _table()}
