"""The check of tests/test_gpu_attn_mod.py (the suite's standard tolerance against the float64 reference with soft cap and
sinks, tests/attn_ref.py, on the inputs of tests/attn_mod_cases.py) must reject each mistake a kernel could make with the two
score modifiers, on the same inputs and shapes the GPU test runs, and pass the reference computed from the exact code x scale values the kernels work with. CPU
only: a model of each mistake stands in for the kernel."""
import numpy as np
import pytest

from tests import attn_mod_cases as M
from tests.attn_cases import KINDS

# (mode, B, Hq, Hkv, T, S, D, window, kv_start, with_new): the decode shape of DECODE_ROUTES, windowed and padded forms, and
# the two extend launch patterns of tests/test_gpu_attn_adversarial.py
SHAPES = {
    "decode": ("decode", 2, 32, 8, 600, 1, 128, 0, None, True),
    "decode hd64 nq8 window": ("decode", 2, 16, 2, 600, 1, 64, 200, None, True),
    "decode padded": ("decode", 2, 32, 8, 600, 1, 128, 0, [37, 600], True),
    "extend one split": ("extend", 1, 32, 8, 128, 16, 128, 0, None, True),
    "extend splits": ("extend", 1, 32, 8, 1000, 16, 128, 0, None, True),
}
CAP_MISTAKES = ("cap_skip_new", "cap_after_max", "cap_before_scale")
SINK_MISTAKES = ("sink_by_kv_head", "sink_not_in_max", "sink_value_row", "sink_per_split")


def _case(name, dtype="f16", amp=1.0):
    mode, B, Hq, Hkv, T, S, D, W, ks, with_new = SHAPES[name]
    return M.make_mod_case(mode, B, Hq, Hkv, T, S, D, KINDS, dtype, seed=len(name), with_new=with_new, window=W, kv_start=ks,
                           amp=amp)


@pytest.mark.parametrize("name", list(SHAPES))
def test_softcap_inputs_have_the_shares_the_design_asks_for(name):
    """a share of every row's keys at |s| >= 2 c, the rest below c / 4, nothing in between"""
    big, small, between = M.score_shares(_case(name))
    assert 0.1 <= big <= 0.4 and small >= 0.6 and between == 0.0, (big, small, between)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_modifiers_move_the_result_far_beyond_the_tolerance(name, dtype):
    c, cs = _case(name, dtype), _case(name, dtype, amp=M.SINK_AMP)
    ok, r = M.check(M.reference(c), M.reference(c, softcap=M.CAP), dtype)
    assert not ok and r > 10, r  # an order of magnitude past the tolerance
    sinks = M.make_sinks(cs)
    ok, r = M.check(M.reference(cs), M.reference(cs, sinks=sinks), dtype)
    assert not ok and r > 10, r
    # the kernels multiply exact codes by the scales where the reference rounds the dequantised value: inside the tolerance
    for cc, kw in ((c, dict(softcap=M.CAP)), (cs, dict(sinks=sinks)), (c, dict(softcap=M.CAP, sinks=M.make_sinks(c, M.CAP)))):
        ok, r = M.check(M.reference(cc, exact=True, **kw), M.reference(cc, **kw), dtype)
        assert ok and r < 0.5, (kw.keys(), r)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("mistake", CAP_MISTAKES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_check_rejects_softcap_mistakes(name, mistake, dtype):
    c = _case(name, dtype)
    for sinks in (None, M.make_sinks(c, M.CAP)):
        ref = M.reference(c, softcap=M.CAP, sinks=sinks)
        ok, r = M.check(M.reference(c, softcap=M.CAP, sinks=sinks, mistake=mistake, exact=True), ref, dtype)
        assert not ok, (name, mistake, sinks is not None, r)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("mistake", SINK_MISTAKES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_check_rejects_sink_mistakes(name, mistake, dtype):
    for cap in (0.0, M.CAP):
        c = _case(name, dtype, amp=1.0 if cap else M.SINK_AMP)
        sinks = M.make_sinks(c, cap)
        ref = M.reference(c, softcap=cap, sinks=sinks)
        ok, r = M.check(M.reference(c, softcap=cap, sinks=sinks, mistake=mistake, exact=True), ref, dtype)
        assert not ok, (name, mistake, cap, r)


def test_sink_kinds():
    """per head: above every score, equal to the top score, -1e30 (no effect), half the mass"""
    c = _case("decode")
    sinks = M.make_sinks(c)
    s = M.scores(c)[0, :, -1]
    top = s.max(axis=-1)
    assert np.allclose(sinks[0::4], top[0::4] + 3.0) and np.allclose(sinks[1::4], top[1::4]) and (sinks[2::4] == np.float32(-1e30)).all()
    with_s, without = M.reference(c, sinks=sinks), M.reference(c)
    # a -1e30 sink changes nothing; a sink at the log-sum-exp halves the row (batch row 0, whose scores it was built from)
    assert np.array_equal(with_s[:, 2::4], without[:, 2::4])
    assert np.allclose(with_s[0, 3::4], 0.5 * without[0, 3::4], rtol=1e-5, atol=1e-9)


def test_row_without_a_key_is_zeros_with_and_without_a_sink():
    mode, B, Hq, Hkv, T, S, D, W, _, _ = SHAPES["decode"]
    c = M.make_mod_case(mode, B, Hq, Hkv, T, S, D, KINDS, "f16", seed=3, with_new=False, kv_start=[37, T])
    for kw in (dict(), dict(softcap=M.CAP), dict(sinks=M.make_sinks(c)), dict(softcap=M.CAP, sinks=M.make_sinks(c, M.CAP))):
        ref = M.reference(c, **kw)
        assert (ref[1] == 0).all() and np.abs(ref[0]).max() > 0
