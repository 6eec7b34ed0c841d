"""CPU proof that the quantise edge families (tests/quant_cases.py) can catch the mistakes a quantise kernel can make.

The GPU tests in test_gpu_quant_edges.py compare every route with the oracle, byte for byte, on these families. That only
means something if the families reach the places where a kernel could be subtly wrong. Here the exact emulation of the
vector kernels' quotient (``quant_cases.emulate_quant``) stands in for the kernel:

  - with its guard fallback and its clamp it equals the oracle on every family (so the emulation is faithful);
  - without the fallback it differs on the tie families (exact ties and the guard band need the IEEE redo);
  - without the clamp it differs on the small-table families, with a corrupted INT4 neighbour nibble among them;
  - rounding half away from zero, and rounding RN(x * RN(1/s32)) without the guard, are both rejected.

The non-finite family (``quant_cases.nonfinite_cases``) is checked the same way against ``quant_cases.contract_quant``,
a slice-by-slice statement of the contract: unmodified it equals the oracle on every case, and each mistake a kernel can
make with a NaN or an inf (a value maximum that drops the NaN, an eps floor that swallows a NaN scale, a NaN quotient
clamped to QMIN, an INT4 nibble of 0 for a non-finite product, an accumulating abs-max that forgets the table's NaN, a
poisoned token that leaks into its neighbour's scale) fails on at least one case.

It also asserts the counts that make the families worth running (exact ties, guard-band vectors, eps-floor tokens,
clamped elements), so that none of them drops to zero unnoticed.
"""
import numpy as np
import pytest

from tests import quant_cases as C

SHAPE = (2, 1, 8, 16, 128)      # the Llama row shape; 32 tokens of 1,024 elements
DTYPES = ("f16", "bf16", "f32")


def _families(dtype, kind):
    return C.quant_cases(SHAPE, dtype, kind, given_table=True, max_chunks=3)


def _same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8))


@pytest.fixture(scope="module")
def families():
    return {(dt, k): _families(dt, k) for dt in DTYPES for k in C.KINDS}


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_emulation_equals_oracle(families, dtype, kind):
    for case in families[dtype, kind]:
        q_ref, s_ref = C.reference(case, kind)
        q, s = C.emulate_quant(case, kind)
        assert _same(q, q_ref), case.name
        assert _same(s, s_ref), case.name


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_no_fallback_is_caught(families, dtype, kind):
    """Without the IEEE-divide redo the fused rounding alone differs wherever x * RN(1/s32) is on the wrong side of a
    half-integer: at exact ties with an inexact reciprocal, and in the guard band."""
    caught = [c.name for c in families[dtype, kind]
              if "ties" in c.tags and not _same(C.emulate_quant(c, kind, fallback=False)[0], C.reference(c, kind)[0])]
    assert caught, "no tie case tells a quotient without its fallback from the reference"


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_no_clamp_is_caught(families, dtype, kind):
    """A table below the data's maximum makes quotients beyond QMAX: without the clamp the stored byte is the magic
    sum's low byte (INT8 -254 -> +2), and an INT4 code past 15 spills into its even neighbour's nibble."""
    caught, neighbour = [], False
    for c in families[dtype, kind]:
        if "table" not in c.tags:
            continue
        q_ref = C.reference(c, kind)[0]
        q = C.emulate_quant(c, kind, clamp=False)[0]
        if _same(q, q_ref):
            continue
        caught.append(c.name)
        if kind == "int4":
            # an even element whose own code byte is in range, yet its stored nibble is wrong: the odd neighbour's
            # byte (above 15) spilled into it
            s32 = C.scale32(c.table, kind, c.eps)[:, None, None, :, None]
            b = C.emulate_quotient(C.widen(c.x, c.dtype), s32, kind, clamp=False) & 0xFF
            spill = (b[..., 1::2] > 15) & (b[..., 0::2] <= 15) & ((q >> 4) != (q_ref >> 4))
            neighbour |= bool(spill.any())
    assert {"table_half", "table_zero"} <= set(caught), caught
    for c in families[dtype, kind]:
        if "table" not in c.tags or c.name in ("table_half", "table_zero", "table_ulp_down"):
            continue
        assert c.name not in caught, c.name  # at or above the data's maximum the clamp never fires
    if kind == "int4":
        assert neighbour, "no INT4 case shows a corrupted neighbour nibble"


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("dtype", ("f16", "f32"))
@pytest.mark.parametrize("mutation", ["away", "unfused"])
def test_rounding_mutations_are_caught(families, dtype, kind, mutation):
    sw = {"away": {"away": True}, "unfused": {"fused": False}}[mutation]
    caught = [c.name for c in families[dtype, kind] if not _same(C.emulate_quant(c, kind, **sw)[0], C.reference(c, kind)[0])]
    if mutation == "away":  # every exact tie with an odd k + 1/2 tells the two roundings apart
        assert any(n.startswith("tie_") for n in caught) and any(n.startswith("exh_") for n in caught), caught
    elif dtype == "f32":    # RN(x * r) lands ON k + 1/2 from just below it: the fp32 near-ties of the guard band
        assert any(n.startswith("tie_") for n in caught), caught
    else:                   # a 2-byte dtype has no values that close to a tie; random data still shows it
        assert caught, caught


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_families_reach_their_edges(families, dtype, kind):
    """Per family: exact ties, guard-band vectors, eps-floor tokens and clamped elements must not silently vanish."""
    tot = {}
    for c in families[dtype, kind]:
        fam = c.name.split("_")[0]
        st = C.stats(c, kind)
        for k, v in st.items():
            tot[fam, k] = tot.get((fam, k), 0) + v
        if c.name == "table_half" or c.name == "table_zero":
            assert st["clamp"] > 0, (c.name, st)
        if c.name == "table_zero":
            assert st["eps_floor"] > 0, (c.name, st)
        if c.name in ("table_equal", "table_ulp_up", "table_double"):
            assert st["clamp"] == 0, (c.name, st)
        if c.name == "eps_0.25":
            assert st["eps_floor"] == SHAPE[0] * SHAPE[3], (c.name, st)
        if c.name == "eps_0.001":
            assert 0 < st["eps_floor"] < SHAPE[0] * SHAPE[3], (c.name, st)
    assert tot["tie", "ties"] > 0 and tot["tie", "guard"] > 0, tot
    assert tot["exh", "guard"] > 0, tot
    if dtype == "f16" or (dtype == "f32"):
        assert tot["exh", "ties"] > 0, tot
        assert tot["exh", "eps_floor"] > 0, tot
    assert tot["exh", "clamp"] == 0 and tot["tie", "clamp"] == 0 and tot["probe", "clamp"] == 0, tot


def test_int8_no_clamp_example():
    """The issue's worked example: s32 = 1/127, x = -2 gives a quotient of -254; the magic sum's low byte is 0x02."""
    s = np.float32(1) / np.float32(127)
    x = np.full((1, 8), -2.0, np.float32)
    raw = C.pack_bytes(C.emulate_quotient(x, s, "int8", clamp=False), "int8")
    ok = C.pack_bytes(C.emulate_quotient(x, s, "int8"), "int8")
    assert raw[0, 0] == 2 and ok[0, 0] == -127


def test_dequant_code_cases_cover_every_byte():
    for kind in C.KINDS:
        for out in ("f16", "bf16", "f32"):
            (_, q, s), (_, qb, sb) = C.dequant_code_cases(kind, out)
            assert len(np.unique(qb.view(np.uint8))) == 256 and np.isnan(sb).any() and np.isposinf(sb).any() and np.isneginf(sb).any()
            assert len(np.unique(q.view(np.uint8))) == 256
            assert (s == 0).any() and np.signbit(s[s == 0]).any() and (~np.signbit(s[s == 0])).any()
            # some products are exact ties of the output dtype (halfway between two neighbours), so RN-even decides them
            if out != "f32":
                codes = (q.view(np.int8).astype(np.float64) if kind == "int8"
                         else (np.stack([q >> 4, q & 0xF], -1).astype(np.float64) - 8))
                prod = np.unique(codes)[:, None] * s.astype(np.float64).reshape(-1)[None, :]
                prod = prod[np.isfinite(prod) & (prod != 0) & (np.abs(prod) < 1e4)]
                m, _ = np.frexp(np.abs(prod))                      # significand in [1/2, 1)
                y = m * 2.0 ** ((11 if out == "f16" else 8) + 1)   # one bit past the output's significand
                assert ((y == np.floor(y)) & (y % 2 == 1)).any(), (kind, out)


# ------------------------------------------------------------------------------------------------ non-finite inputs
NF_SHAPES = [(2, 1, 8, 16, 128), (1, 16, 8, 4, 128), (2, 1, 4, 3, 7), (2, 4, 8, 1, 128)]  # tile, parts, odd D, one token


@pytest.fixture(scope="module")
def nonfinite():
    return {(sh, dt, k): C.nonfinite_cases(sh, dt, k, given_table=True) for sh in NF_SHAPES for dt in DTYPES for k in C.KINDS}


def _nf_differs(case, kind, **mistake):
    q_ref, s_ref = C.reference(case, kind)
    q, s = C.contract_quant(case, kind, **mistake)
    return not (_same(q, q_ref) and C.same_floats(s, s_ref))


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_nonfinite_contract_equals_oracle(nonfinite, dtype, kind):
    """The contract stated slice by slice is what the oracle computes, and the family is what it claims to be: every
    poison, every position, clean tokens next to poisoned ones, tables of every class."""
    for sh in NF_SHAPES:
        G, B, H, T, D = sh
        cases = nonfinite[sh, dtype, kind]
        assert {c.name for c in cases} >= {f"nonfinite_{p}" for p in C.POISONS}
        seen, mixed = set(), False
        for c in cases:
            assert not _nf_differs(c, kind), (sh, c.name)
            q, s = C.reference(c, kind)
            am = C.data_absmax(c.x, c.dtype)
            assert C.same_floats(C.contract_absmax(c.x, c.dtype), am)
            bad = ~np.isfinite(C.widen(c.x, c.dtype)).all(axis=(1, 2, 4))                       # [G, T] poisoned slices
            u = C.raw_bits(c.x, c.dtype).reshape(G, B * H, T, D)
            fin = (u & (C.SIGN_BIT[c.dtype] - 1)) < C.INF_BITS[c.dtype]
            seen |= {(int(r), int(d)) for _, r, _, d in np.argwhere(~fin)}
            if c.table is None:
                assert bad.any() and (T < 5 or (~bad).any()), c.name
                mixed |= bool((~bad).any())
                zero = 0x88 if kind == "int4" else 0
                assert (np.moveaxis(q, 3, 1)[bad].view(np.uint8) == zero).all(), c.name         # every code of a poisoned slice
                assert (C.absmax_class(s)[bad] == C.absmax_class(am)[bad]).all() and (C.absmax_class(s)[~bad] == 0).all()
                if "nan" in c.name:
                    assert np.isnan(s[bad]).all(), c.name                                      # NaN wins over inf
                clean = C.Case("clean", C.gaussian_base(sh, dtype), dtype)
                qc, sc = C.reference(clean, kind)
                assert _same(np.moveaxis(q, 3, 1)[~bad], np.moveaxis(qc, 3, 1)[~bad]) and _same(s[~bad], sc[~bad]), c.name
        assert seen >= set(C.slice_positions(sh)), (sh, seen)
        assert mixed or T < 2, sh   # T of 3 or 4: every other case keeps a clean token between the poisoned ends
        if B * H * D > 8192:
            assert {"nonfinite_piece_first", "nonfinite_piece_last"} <= {c.name for c in cases}


MISTAKES = [("drop_nan", {"drop_nan": True}), ("eps_swallows_nan", {"drop_nan": False, "eps_swallows_nan": True}),
            ("nan_as_qmin", {"nan_as_qmin": True}), ("nibble_zero", {"nibble_zero": True}), ("leak", {"leak": True})]


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mistake", MISTAKES, ids=[m[0] for m in MISTAKES])
def test_nonfinite_mistakes_are_caught(nonfinite, dtype, kind, mistake):
    name, sw = mistake
    for sh in NF_SHAPES:
        caught = [c.name for c in nonfinite[sh, dtype, kind] if _nf_differs(c, kind, **sw)]
        if name == "nibble_zero" and kind == "int8":  # an INT4 mistake: the INT8 byte of a non-finite magic sum is 0, the right code
            assert not caught, (sh, caught)
            continue
        if name == "leak" and sh[3] < 2:  # one token per group: no neighbour to leak into
            assert not caught, (sh, caught)
            continue
        assert caught, (sh, name)
        if name in ("drop_nan", "eps_swallows_nan"):   # every NaN poison tells; the inf poisons need neither
            assert {f"nonfinite_{p}" for p in ("qnan", "neg_nan", "snan", "nan_inf")} <= set(caught), (sh, caught)
        if name == "nan_as_qmin":                       # a NaN element under a finite caller-given scale, too
            assert any(n.startswith("nonfinite_table_") for n in caught), (sh, caught)
        if name == "leak" and sh[3] >= 2:               # a clean right neighbour exists
            assert len(caught) >= 3, (sh, caught)


@pytest.mark.parametrize("dtype", DTYPES)
def test_nonfinite_absmax_acc_mistakes_are_caught(dtype):
    """kvq_absmax_tokens_acc onto a table that holds NaN, +inf and finite entries: the table's NaN stays, data NaN enters,
    +inf is a value. fmaxf(old, new) forgets the table's NaN (and drops the data's); a value maximum drops the data's."""
    sh = (2, 4, 8, 3, 128)
    for case in C.nonfinite_cases(sh, dtype, "int8", given_table=False):
        old = np.array([[np.nan, np.inf, 0.5], [1e9, np.nan, np.inf]], np.float32)
        ref = np.maximum(old, C.data_absmax(case.x, case.dtype))
        assert C.same_floats(C.contract_absmax(case.x, dtype, old), ref)
        assert np.isnan(ref[0, 0]) and np.isnan(ref[1, 1])
        assert not C.same_floats(C.contract_absmax(case.x, dtype, old, forget_nan=True), ref), case.name
    nan_cases = [c for c in C.nonfinite_cases(sh, dtype, "int8", given_table=False) if "nan" in c.name]
    for case in nan_cases:
        assert not C.same_floats(C.contract_absmax(case.x, dtype, drop_nan=True), C.data_absmax(case.x, dtype)), case.name


def test_float_mismatch_rule():
    """any NaN for a NaN of the reference's; bits everywhere else: +inf is not -inf, +0 is not -0, a NaN is not an inf"""
    ref = np.array([np.nan, np.inf, 0.0, 1.0], np.float32)
    ok = np.array([0xFFC00001, 0x7F800000, 0, 0x3F800000], np.uint32).view(np.float32)
    assert C.same_floats(ok, ref)
    for i, b in ((0, 0x7F800000), (1, 0xFF800000), (1, 0x7FC00000), (2, 0x80000000), (3, 0x3F800001)):
        bad = ok.copy().view(np.uint32)
        bad[i] = b
        assert C.float_mismatch(bad.view(np.float32), ref, "f32").tolist() == [j == i for j in range(4)]
    h = np.array([0x7E00, 0xFC00], np.uint16)
    assert C.same_floats(np.array([0xFE01, 0xFC00], np.uint16).view(np.float16), h.view(np.float16), "f16")
    assert C.same_floats(np.array([0x7FC1, 0xFF80], np.uint16), np.array([0xFFC0, 0xFF80], np.uint16), "bf16")
    assert not C.same_floats(np.array([0x7F80, 0xFF80], np.uint16), np.array([0xFFC0, 0xFF80], np.uint16), "bf16")
