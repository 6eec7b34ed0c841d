"""Logit soft-capping and attention sinks in the kernels (the ``kvq_*_ex`` entry points) against the float64
reference of tests/attn_ref.py under the suite's standard tolerance, for {cap, sinks, both} on every decode route of
tests/attn_cases.py::DECODE_ROUTES (plus INT4 keys on the one-tile route) through kvq_decode_attn_ex (with and
without a new token), kvq_decode_step_ex (slot T bit-identical to kvq_decode_step's) and kvq_decode_step_dev_ex (a count
below its bound), with and without a window that cuts, with kv_start NULL and given (one row that sees no stored key), and
on both extend launch patterns (a banded chunk, S > W, among them), in f16 and bf16. Every test reads the kernel log: the
``_mod_k`` kernels with a modifier on, the unmodified ones with both off. tests/test_attn_mod_discrimination.py shows that
the same check rejects the mistakes that matter on the same inputs."""
import contextlib

import numpy as np
import pytest
import torch

from tests import attn_mod_cases as M
from tests.attn_cases import DECODE_ROUTES, EXTEND_ROUTES, KINDS
from tests.gpu_harness import K, run_case, tunable  # noqa: F401

pytestmark = pytest.mark.gpu

MODS = ("cap", "sinks", "both")
ROUTES = {name: (shape, knobs, kernel.split("_k<")[0], KINDS) for name, (shape, knobs, kernel, _) in DECODE_ROUTES.items()}
ROUTES["one-tile MFMA INT4 K"] = ((2, 32, 8, 600, 128), {"attn_stream_tpw": -1}, "decode_attn_partial_mfma", ("int4", "int4"))
DEV_SPARE = 37  # the device-count step runs at count T under the bound T + 37


@contextlib.contextmanager
def forced_ex(K, softcap=None, null_opts=False):
    """Every call of kernels.* goes through its ``_ex`` entry point, also with both modifiers off; ``softcap``: that value
    in the record instead of the call's (past the Python-side validation); ``null_opts``: a NULL record."""
    from efficient_llm_inference_amd import _lib
    orig = K._windowed_entry

    def entry(lib, base, window, kv_start_p, cap=0.0, sinks_p=None):
        if null_opts:
            return getattr(lib, base + "_ex"), (None,)
        opts = _lib.KvqAttnOpts(window, None if kv_start_p is None else kv_start_p.value, cap if softcap is None else softcap,
                                None if sinks_p is None else sinks_p.value)
        return getattr(lib, base + "_ex"), (_lib.byref(opts),)
    K._windowed_entry = entry
    try:
        yield
    finally:
        K._windowed_entry = orig


def run(K, c, entry, softcap=0.0, sinks=None):
    """Case ``c`` through one entry point (tests/gpu_harness.py::run_case). Returns (float64 result, kernel log, slot T of the
    stores afterwards as numpy: K row, V row, scales)."""
    got, log, stores = run_case(K, c, entry, softcap=softcap, sinks=sinks, bound=c.T + DEV_SPARE if entry == "dev" else None,
                                cap=c.T + DEV_SPARE + 8)
    return got, log, stores.slot(c.T)


def mods_of(c, mod):
    """(softcap, sinks) of a modifier set for case c"""
    cap = M.CAP if mod in ("cap", "both") else 0.0
    return cap, (M.make_sinks(c, cap) if mod in ("sinks", "both") else None)


def case(mode, shape, kinds, dtype, mod, seed, **kw):
    B, Hq, Hkv, T, S, D = shape
    return M.make_mod_case(mode, B, Hq, Hkv, T, S, D, kinds, dtype, seed=seed, amp=M.SINK_AMP if mod == "sinks" else 1.0, **kw)


def assert_mod_log(log, base_log, mod, family=None):
    """the kernel log of a modified call against the same call's without modifiers: a soft cap takes the family's capped
    partial kernel, sinks alone keep the partial kernel of the plain call; the merge is a ``_mod_k`` one either way"""
    assert not any("_mod_k" in k for k in base_log), base_log
    assert len(log) == 2 and "_mod_k" in log[1] and "merge" in log[1], (log, base_log)
    if mod == "sinks":
        assert log[0] == base_log[0], (log, base_log)
    else:
        assert "_mod_k<" in log[0] and (family is None or log[0].startswith(family + "_mod_k<")), (log, family)


def within(c, got, softcap, sinks, what):
    ref = M.reference(c, softcap, sinks)
    ok, r = M.check(got, ref, c.dtype)
    assert ok, (what, c.dtype, r)
    if c.kv_start is not None:  # a row that sees no key: exactly zero
        dead = ~M._visible(c).any(axis=-1)  # [B,S]
        g = got[:, :, None] if c.mode == "decode" else got
        assert (g.transpose(0, 2, 1, 3)[dead] == 0).all(), what
    return r


# (with the new token, window: None = none / "cut" = a third of T, kv_start: None or per-row starts from T)
def decode_variants(B, T):
    rest = [37, 100, 5, 64][: B - 1]
    return [(True, 0, None), (False, T // 3, None), (True, T // 3, [T] + rest), (False, 0, rest[:1] + [T] + rest[1:])]


@pytest.mark.parametrize("mod", MODS)
@pytest.mark.parametrize("route", list(ROUTES))
def test_decode_attn_ex_routes(K, tunable, route, mod):
    (B, Hq, Hkv, T, D), knobs, family, kinds = ROUTES[route]
    for key, val in knobs.items():
        tunable(key, val)
    for i, (with_new, W, starts) in enumerate(decode_variants(B, T)):
        dtype = ("f16", "bf16")[i % 2] if kinds == KINDS else "f16"
        c = case("decode", (B, Hq, Hkv, T, 1, D), kinds, dtype, mod, seed=len(route) + i, with_new=with_new, window=W, kv_start=starts)
        cap, sinks = mods_of(c, mod)
        _, base_log, _ = run(K, c, "attn")
        got, log, _ = run(K, c, "attn", cap, sinks)
        assert_mod_log(log, base_log, mod, family if i == 0 else None)
        within(c, got, cap, sinks, (route, mod, with_new, W, starts))


@pytest.mark.parametrize("mod", MODS)
@pytest.mark.parametrize("route", list(ROUTES))
def test_decode_step_ex_and_step_dev_ex(K, tunable, route, mod):
    """the step entry points: the attention against the reference, slot T bit-identical to the unmodified step's"""
    (B, Hq, Hkv, T, D), knobs, family, kinds = ROUTES[route]
    for key, val in knobs.items():
        tunable(key, val)
    for i, (entry, W, starts, dtype) in enumerate((("step", 0, None, "bf16"), ("step", T // 3, [T, 37], "f16"),
                                                   ("dev", 0, None, "f16"), ("dev", T // 3, [41, T], "bf16"))):
        c = case("decode", (B, Hq, Hkv, T, 1, D), kinds, dtype, mod, seed=len(route) + 10 + i, window=W, kv_start=starts)
        cap, sinks = mods_of(c, mod)
        _, base_log, base_slot = run(K, c, entry)
        got, log, slot = run(K, c, entry, cap, sinks)
        assert_mod_log(log, base_log, mod)
        within(c, got, cap, sinks, (route, mod, entry, W, starts))
        for a, b in zip(slot, base_slot):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (route, mod, entry)
        assert np.isfinite(slot[2]).all() and np.isfinite(slot[3]).all()  # the slot was written (NaN before)


EXT_SHAPES = {  # name -> ((B, Hq, Hkv, T, S, D), window, kv_start, merge expected)
    "one split": (EXTEND_ROUTES["one split"][0], 0, None, False),
    "splits + merge": (EXTEND_ROUTES["splits + merge"][0], 0, None, True),
    "one split, banded chunk": ((1, 32, 8, 128, 40, 128), 24, None, False),
    "splits + merge, window, padded": ((2, 32, 8, 1000, 16, 128), 700, [1009, 520], True),
    "head_dim 64": (EXTEND_ROUTES["head_dim 64, nq 3"][0], 0, [0, 130], None),
}


@pytest.mark.parametrize("mod", MODS)
@pytest.mark.parametrize("name", list(EXT_SHAPES))
def test_extend_attn_ex(K, name, mod):
    shape, W, starts, merge = EXT_SHAPES[name]
    for dtype in ("f16", "bf16"):
        c = case("extend", shape, KINDS, dtype, mod, seed=len(name), window=W, kv_start=starts)
        cap, sinks = mods_of(c, mod)
        _, base_log, _ = run(K, c, "extend")
        got, log, _ = run(K, c, "extend", cap, sinks)
        assert not any("_mod_k" in k for k in base_log), base_log
        assert log[0].startswith("extend_attn_mod_k<") and len(log) == len(base_log), (log, base_log)
        if merge is not None:
            assert (len(log) == 2) == merge, log
        assert len(log) == 1 or log[1].startswith("extend_attn_merge_mod_k<"), log
        within(c, got, cap, sinks, (name, mod))


@pytest.mark.parametrize("entry", ["attn", "step", "dev", "extend"])
def test_ex_with_both_off_is_the_padded_call(K, tunable, entry):
    """same kernels in the log, same bits: without and with kv_start, without and with a window"""
    tunable("attn_stream_tpw", 2)
    shape = (2, 32, 8, 1000, 16, 128) if entry == "extend" else (2, 32, 8, 600, 1, 128)
    T = shape[3]
    for W, starts in ((0, None), (T // 3, None), (0, [T // 2, 3]), (T // 3, [T - 7, 0])):
        c = case("extend" if entry == "extend" else "decode", shape, KINDS, "f16", "cap", seed=W + 1, window=W, kv_start=starts)
        want, want_log, want_slot = run(K, c, entry)
        with forced_ex(K):
            got, log, slot = run(K, c, entry)
        assert log == want_log and not any("_mod_k" in k for k in log), (log, want_log)
        assert np.array_equal(got, want), (entry, W, starts)
        for a, b in zip(slot, want_slot):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (entry, W, starts)


@pytest.mark.parametrize("route", ["one-tile MFMA", "ring hd128 TG4", "VALU hd32"])
def test_a_sink_of_minus_1e30_equals_no_sink(K, tunable, route):
    (B, Hq, Hkv, T, D), knobs, family, kinds = ROUTES[route]
    for key, val in knobs.items():
        tunable(key, val)
    for cap in (0.0, M.CAP):
        c = case("decode", (B, Hq, Hkv, T, 1, D), kinds, "f16", "both" if cap else "sinks", seed=9)
        got, log, _ = run(K, c, "attn", cap, np.full(Hq, -1e30, np.float32))
        assert "_mod_k" in log[1], log
        ok, r = M.check(got, M.reference(c, cap, None), "f16")
        assert ok, (route, cap, r)
    if D in (64, 128):
        ce = case("extend", (1, Hq, Hkv, T, 16, D), kinds, "f16", "sinks", seed=9)
        got, log, _ = run(K, ce, "extend", 0.0, np.full(Hq, -1e30, np.float32))
        assert log[0].startswith("extend_attn_mod_k<"), log
        ok, r = M.check(got, M.reference(ce), "f16")
        assert ok, (route, r)


def test_argument_errors(K):
    from efficient_llm_inference_amd import _lib
    c = case("decode", (2, 32, 8, 600, 1, 128), KINDS, "f16", "cap", seed=1)
    ce = case("extend", (1, 32, 8, 128, 16, 128), KINDS, "f16", "cap", seed=1)
    for cc, entries in ((c, ("attn", "step", "dev")), (ce, ("extend",))):
        for entry in entries:
            with forced_ex(K, null_opts=True), pytest.raises(_lib.KvqError, match="NULL opts"):
                run(K, cc, entry)
            for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
                with forced_ex(K, softcap=bad), pytest.raises(_lib.KvqError, match="softcap"):
                    run(K, cc, entry)
    # the Python layer refuses them before the library is called
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(_lib.KvqError, match="softcap"):
            run(K, c, "attn", softcap=bad)
    with pytest.raises(_lib.KvqError, match="sinks"):
        run(K, c, "attn", sinks=np.zeros(c.Hq + 1, np.float32))
    half = torch.zeros(c.Hq, dtype=torch.float16, device="cuda")
    with pytest.raises(_lib.KvqError, match="float32"):
        K._sinks_arg(half, c.Hq, half.device, "decode_attn")
