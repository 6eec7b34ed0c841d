"""CPU: the float64 model of kvq_key_scores (tests/key_score_cases.key_mass) is the header's formula, and the suite's
tolerance on it rejects wrong kernels.

(a) the model equals tests/attn_ref.attention run with V = identity (D keys): the output row IS the probability row;
(b) every probability row sums to 1, so a kv head's mass sums to nq * S;
(c) discrimination: each deliberate mistake moves some element by >= 5x the limit ``TOL * (|ref| + max |ref|)`` the GPU test
    applies, in the family and shape designated for it. The designated cases are fp16 (bf16's limit is 8x wider: the same
    kernel text serves both dtypes, so a mistake fp16 convicts cannot hide in bf16). Ratios measured with this file::

        causal bound +1                     flat (2,4,1,130,16,64) 72x    flat (1,8,2,321,17,128) 34x
        causal bound -1                     flat (2,4,1,130,16,64) 101x   flat (1,8,2,321,17,128) 28x
        token 64 dropped                    flat 182x / 188x, probe 234x / 250x, scale_span 81x / 52x
        first window token T - S dropped    flat 191x / 186x, probe 250x / 250x, scale_span 81x / 52x
        normaliser over all T               flat (2,4,1,130,16,64) 18x    flat (1,8,2,321,17,128) 7.6x
        head map h % Hkv                    flat (1,8,2,321,17,128) 148x
        head 1 of a group left out          flat (2,4,1,130,16,64) 90x    flat (1,8,2,321,17,128) 145x
        k_scales[t + 1] used for t          scale_span int4 (2,4,1,130,16,64) 694x    int8 (1,8,2,321,17,128) 341x
        accumulate overwrites               flat (2,4,1,130,16,64) 200x   flat (1,8,2,321,17,128) 224x
        nibbles swapped                     flat int4 (2,4,1,130,16,64) 148x          (1,8,2,321,17,128) 213x

    Two weaknesses of these designations: the all-T normaliser is only 1.7x at T = 1300 (not designated), and probes on
    identical kv heads do not see the head map (flat does).
Also here: the model on keys rounded to fp16 differs from the exact one by at most 0.08x the limit (asserted: <= 0.25x), so the choice of model is not
what the tolerance absorbs; and the probe family's targets receive the number of rows aimed at them."""
import numpy as np
import pytest

from tests import attn_ref
from tests.attn_cases import widen
from tests.key_score_cases import FAMILIES, key_mass, limit, make_case, plan

SMALL = (2, 4, 1, 130, 16, 64)
WIDE = (1, 8, 2, 321, 17, 128)
_CASES = {}


def case(family, shape, kind="int8", dtype="f16"):
    """one case and its reference per (family, shape, kind, dtype), shared by the tests below"""
    key = (family, shape, kind, dtype)
    if key not in _CASES:
        B, Hq, Hkv, T, S, D = shape
        c = make_case(family, B, Hq, Hkv, T, S, D, kind, dtype, seed=11)
        _CASES[key] = (c, key_mass(c))
    return _CASES[key]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape,kind,dtype", [(SMALL, "int8", "f16"), (WIDE, "int4", "bf16"), ((1, 5, 1, 65, 13, 64), "int8", "bf16")])
def test_model_is_attention_with_identity_values(family, shape, kind, dtype):
    c, ref = case(family, shape, kind, dtype)
    B, Hq, Hkv, T, S, D = shape
    kd = c.kint * c.ks.astype(np.float64)[:, None]
    q = widen(c.q, dtype)
    nq = Hq // Hkv
    mass = np.zeros((B, Hkv, T))
    for t0 in range(0, T, D):  # V = identity over D keys at a time: the output row is the probability row of those keys
        n = min(D, T - t0)
        v = np.zeros((B, Hkv, T, D))
        v[:, :, t0 + np.arange(n), np.arange(n)] = 1.0
        p = attn_ref.attention(q, kd, v, T - S + np.arange(S), c.sm)[..., :n]  # [B,Hq,S,n]
        mass[:, :, t0:t0 + n] += p.reshape(B, Hkv, nq, S, n).sum(axis=(2, 3))
    assert np.abs(mass - ref).max() <= 1e-12 * nq * S


@pytest.mark.parametrize("family", FAMILIES)
def test_mass_sums_to_rows(family):
    for shape in (SMALL, WIDE):
        c, ref = case(family, shape)
        B, Hq, Hkv, T, S, D = shape
        np.testing.assert_allclose(ref.sum(axis=-1), np.full((B, Hkv), (Hq // Hkv) * S), rtol=1e-12)
        assert (ref >= 0).all()


def test_probe_targets_receive_their_rows():
    for shape in (SMALL, WIDE):
        c, ref = case("probe", shape)
        assert c.info["aimed"]
        for (b, g, tok), n in c.info["aimed"].items():
            # the rows aimed at it give it all their weight; only a row aimed at a token it does not see adds to it
            assert n * (1 - 1e-3) <= ref[b, g, tok] <= n + c.info["blind"].get((b, g), 0) + 1e-3, (shape, b, g, tok, n, ref[b, g, tok])
        assert len(c.info["fixed"]) >= 5


def _ratio(c, ref, **mistake):
    return float((np.abs(key_mass(c, **mistake) - ref) / limit(ref, c.dtype)).max())


def _mistakes():
    every = [(f, s) for f in FAMILIES for s in (SMALL, WIDE)]
    flat_both = [("flat", SMALL), ("flat", WIDE)]
    out = []
    for fam, shape in flat_both:
        out += [("causal bound +1", fam, shape, "int8", dict(shift=1)), ("causal bound -1", fam, shape, "int8", dict(shift=-1)),
                ("normaliser over all T", fam, shape, "int8", dict(norm_all=True))]
    for fam, shape in every:
        T, S = shape[3], shape[4]
        out += [("token 64 dropped", fam, shape, "int8", dict(drop=(64,))),
                ("first window token dropped", fam, shape, "int8", dict(drop=(T - S,)))]
    out += [("head map h % Hkv", "flat", WIDE, "int8", dict(headmap="mod")),
            ("head 1 of a group left out", "flat", WIDE, "int8", dict(skip_head=1)),
            ("head 1 of a group left out", "flat", SMALL, "int8", dict(skip_head=1)),
            ("k_scales[t + 1] used for t", "scale_span", WIDE, "int8", dict(scale_next=True)),
            ("k_scales[t + 1] used for t", "scale_span", SMALL, "int4", dict(scale_next=True)),
            ("nibbles swapped", "flat", WIDE, "int4", dict(swap_nibbles=True)),
            ("nibbles swapped", "flat", SMALL, "int4", dict(swap_nibbles=True))]
    return out


@pytest.mark.parametrize("name,family,shape,kind,mistake", _mistakes(), ids=lambda v: v if isinstance(v, str) else None)
def test_check_rejects(name, family, shape, kind, mistake):
    c, ref = case(family, shape, kind)
    r = _ratio(c, ref, **mistake)
    print(f"{name}: {family} {shape} {kind}: {r:.1f}x the limit")
    assert r >= 5.0, (name, family, shape, r)


@pytest.mark.parametrize("shape", [SMALL, WIDE])
def test_check_rejects_an_accumulate_that_overwrites(shape):
    c, _ = case("flat", shape)
    prior = np.random.default_rng(3).uniform(0.0, 2.0, (c.B, c.Hkv, c.T))
    ref = key_mass(c, prior=prior)
    r = float((np.abs(key_mass(c, prior=prior, overwrite=True) - ref) / limit(ref, c.dtype)).max())
    print(f"accumulate overwrites: flat {shape}: {r:.1f}x the limit")
    assert r >= 5.0, r


@pytest.mark.parametrize("family", FAMILIES)
def test_rounded_keys_are_not_what_the_tolerance_absorbs(family):
    for shape, kind in ((SMALL, "int8"), (WIDE, "int8"), (WIDE, "int4")):
        c, ref = case(family, shape, kind)
        r = float((np.abs(key_mass(c, values="rounded") - ref) / limit(ref, c.dtype)).max())
        print(f"rounded keys: {family} {shape} {kind}: {r:.3f}x the limit")
        assert r <= 0.25, (family, shape, kind, r)


def test_plan_restates_the_launch_shapes():
    # (query blocks, splits, tiles per split, runs, tiles per run)
    assert plan(1, 4, 1, 64, 16) == (1, 1, 1, 1, 1)
    assert plan(2, 8, 2, 319, 16) == (1, 3, 2, 5, 1)
    assert plan(1, 8, 2, 1300, 40)[:2] == (3, 11)
    assert plan(4, 8, 8, 2117, 3)[3:] == (17, 2)
    assert plan(1, 32, 8, 32768, 64) == (4, 32, 16, 128, 4)
