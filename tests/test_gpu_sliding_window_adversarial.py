"""Sliding-window attention over the quantised store on adversarial inputs (tests/attn_cases.py with ``window=W``): every
route is checked against the windowed oracle under the error budget of ``attn_cases.bound``, on cases whose positional
probes sit at each row's lower edge (a target at p - W + 1 the row must see, one at p - W it must not) and at the view's
tile and split boundaries, and the route is asserted with the kernel log. tests/test_attn_discrimination.py shows that the
same check rejects an edge moved by one, a missing per-row edge and the chunk's lower edge ignored.

Every case runs twice: once with the stored rows no query sees (the prefix before the view, and every slot past the
count) holding extreme codes and NaN scales, once with extreme codes and scales of 1e30. ``fmaxf`` drops a NaN, so a
kernel that folded a poisoned V scale into its running maximum would pass the NaN run; the 1e30 run catches it, and the
two outputs must be bit-identical (a kernel that never reads those rows cannot tell them apart)."""
import numpy as np
import pytest

from tests import attn_cases as A
from tests.attn_cases import DECODE_ROUTES, KINDS
from tests.gpu_harness import POISON, K, device_stores, run_case, tunable  # noqa: F401

pytestmark = pytest.mark.gpu

# extend: name -> (B, Hq, Hkv, T, S, D), W, dtype, expected split count
WIN_EXTEND = {
    "one split, S < W, lo0 unaligned": ((1, 8, 8, 100, 16, 128), 64, "f16", 1),
    "splits + merge, S > W, head_dim 64, nq 3": ((1, 12, 4, 900, 300, 64), 256, "bf16", 2),
    "nq 7, splits + merge, lo0 unaligned": ((1, 28, 4, 1200, 40, 128), 300, "bf16", 3),
    "nq 1, lo0 tile-aligned": ((1, 8, 8, 1000, 16, 128), 361, "f16", 3),
    "T = 0, S > W, nq 2": ((1, 4, 2, 0, 150, 64), 40, "f16", 1),
    "W = 1, nq 4": ((1, 16, 4, 300, 20, 128), 1, "f16", 1),
}
# the families of a windowed case: (family, make_case keyword arguments)
WIN_FAMILIES = [("probe", {}), ("sink", {}), ("sink", {"variant": "lo"}), ("late", {}), ("vrange", {})]

# device-count windowed step: name -> (B, Hq, Hkv, D), tunables, kernel-log prefix of the partial, of the merge
WIN_DEV = {
    "MFMA window hd128": ((2, 32, 8, 128), {}, "decode_attn_partial_mfma_window_k<", "decode_attn_merge_fast_k<"),
    "MFMA window hd64": ((4, 16, 4, 64), {}, "decode_attn_partial_mfma_window_k<", "decode_attn_merge_fast_k<"),
    "VALU window NQ1": ((8, 8, 8, 32), {}, "decode_attn_partial_window_k<8, 4, 1>", "decode_attn_merge_fast_k<"),
    "VALU window NQ2": ((8, 8, 4, 256), {}, "decode_attn_partial_window_k<8, 4, 2>", "decode_attn_merge_fast_k<"),
    "VALU window NQ4": ((8, 8, 2, 32), {}, "decode_attn_partial_window_k<8, 4, 4>", "decode_attn_merge_fast_k<"),
    "VALU window NQ8": ((8, 8, 1, 256), {}, "decode_attn_partial_window_k<8, 4, 8>", "decode_attn_merge_fast_k<"),
    "ring dev, fast merge": ((4, 16, 4, 128), {"attn_stream_tpw": 2, "attn_ring_dev": 1, "attn_merge_fast": 1},
                             "decode_attn_lds_mfma_k<", "decode_attn_merge_fast_k<"),
    "ring dev, general merge": ((4, 16, 4, 128), {"attn_stream_tpw": 2, "attn_ring_dev": 1, "attn_merge_fast": 0},
                                "decode_attn_lds_mfma_k<", "decode_attn_merge_k"),
}
# windows and counts: t in {W - 1, W, W + 1} (lo = 0, 1, 2); below W - 1 a count where the live split layout changes
# (W = 40 has one split whatever the count: there lo = 65, the view across the first tile boundary)
WIN_DEV_COUNTS = {40: (39, 40, 41, 104), 700: (699, 700, 701, 257), 2000: (1999, 2000, 2001, 1025)}
# the ring routes also at W = 513: the launch is planned for W - 1 = 512 tokens (8 tiles, 4 splits of 2 tiles at
# attn_stream_tpw = 2), and the merge's live-split count must come from t - window_lo (8 tiles, 4 splits), not from t
# (9 tiles: 3 tiles per split, 3 splits: the view's last split, which holds probes, would be dropped)
WIN_DEV_RING_COUNTS = {513: (513, 514)}
HOST_W = {32: 301, 64: 301, 128: 301, 256: 130}  # host-count decode: the window per head_dim (T = 600 / 300: lo unaligned)


def win_dev_cases(route, widths=None):
    """(W, count, family, make_case keyword arguments) of a device-count route: one family per (W, count), in turn.
    ``widths``: only these windows."""
    i = 0
    table = {**WIN_DEV_COUNTS, **(WIN_DEV_RING_COUNTS if "ring" in route else {})}
    for W, counts in table.items():
        if widths is not None and W not in widths:
            continue
        for t in counts:
            fam, extra = WIN_FAMILIES[i % len(WIN_FAMILIES)]
            i += 1
            if extra.get("variant") == "lo" and A.view_lo("decode", t, W) >= t:
                fam, extra = "probe", {}
            yield W, t, fam, extra


def win_dev_case(route, W, t, fam, extra):
    (B, Hq, Hkv, D), _, _, _ = WIN_DEV[route]
    return A.make_case(fam, "decode", B, Hq, Hkv, t, 1, D, KINDS, "f16", seed=W + t + D, splits=(128,), window=W,
                       **extra)


def win_extend_cases(route):
    """the windowed extend cases of a route, and the split count of its view"""
    (B, Hq, Hkv, T, S, D), W, dtype, _ = WIN_EXTEND[route]
    lo0 = A.view_lo("extend", T, W)
    _, ns, per = A.extend_plan(B, Hq, Hkv, T - lo0, S)
    cases = [A.make_case(fam, "extend", B, Hq, Hkv, T, S, D, KINDS, dtype, seed=T + S + W, splits=(per * 64,) if ns > 1 else (),
                         window=W, **extra)
             for fam, extra in WIN_FAMILIES if not (extra.get("variant") == "lo" and lo0 >= T)]
    return cases, ns


def host_window_cases(route):
    (B, Hq, Hkv, T, D), _, _, splits = DECODE_ROUTES[route]
    W = HOST_W[D]
    return [A.make_case("probe", "decode", B, Hq, Hkv, T, 1, D, KINDS, "f16", seed=T + W, splits=splits, with_new=with_new,
                        window=W) for with_new in ((True, False) if route == "VALU hd32" else (True,))]


def _check(c, got, qplanes, what, ref=None, bud=None):
    if ref is None:
        ref = c.reference()
        bud = A.bound(c, ref, qplanes=qplanes)
    ok, r = A.check(got, ref, bud)
    assert ok, (what, c.info["family"], c.info["variant"], c.dtype, c.T, c.window, r)


def _twice(K, c, entry, log_ok, qplanes, what, **kw):
    """Case ``c`` through ``entry`` on stores whose rows before c.lo and past T hold each poison in turn: the kernel log as
    ``log_ok`` asserts it, each result within budget, the two bit-identical"""
    got = []
    cap = kw["bound"] + 8 if "bound" in kw else c.T + 3
    for poison in POISON.values():
        g, log, _ = run_case(K, c, entry, stores=device_stores(K, c, cap, poison, hide=c.lo), **kw)
        log_ok(log)
        got.append(g)
    ref = c.reference()
    bud = A.bound(c, ref, qplanes=qplanes)
    for g in got:
        _check(c, g, qplanes, what, ref, bud)
    assert np.array_equal(got[0], got[1]), (what, c.info["family"], c.T, c.window, "NaN and 1e30 poison differ")
    return got[0]


@pytest.mark.parametrize("route", list(WIN_EXTEND))
def test_extend_window_on_adversarial_inputs(K, route):
    cases, ns = win_extend_cases(route)
    assert ns == WIN_EXTEND[route][3], (route, ns)
    for c in cases:

        def log_ok(log):
            assert log[0].startswith("extend_attn_window_k<") and (
                log[1:] == [] if ns == 1 else log[1].startswith("extend_attn_merge_k<")), (route, log)
        _twice(K, c, "extend", log_ok, False, route)


@pytest.mark.parametrize("route", list(WIN_DEV))
def test_device_count_window_step_on_adversarial_inputs(K, tunable, route):
    """kvq_decode_step_dev_window: the first visible row derived on the device from the count (window_lo), the one-tile
    window kernels / the ring kernel's device-count instantiation adding it to their row base, and the merge counting the
    live splits from t - window_lo. One family per (W, count), in turn."""
    _, knobs, partial, merge = WIN_DEV[route]
    for key, val in knobs.items():
        tunable(key, val)
    mfma = "mfma" in partial or "lds" in partial
    for W, t, fam, extra in win_dev_cases(route):
        c = win_dev_case(route, W, t, fam, extra)

        def log_ok(log):
            assert log[0].startswith(partial) and log[1].startswith(merge), (route, W, t, log)
            if "lds" in partial:  # the device-count instantiations of the ring kernel and of the fast merge
                assert log[0].endswith(", true>") and (log[1].endswith("true>") or "fast" not in merge), (route, log)
        _twice(K, c, "dev", log_ok, mfma, f"{route} W={W} t={t}", bound=t + 70)


@pytest.mark.parametrize("route", list(DECODE_ROUTES))
def test_host_count_window_decode_view_edges(K, tunable, route):
    """kvq_decode_attn_window: the host moves the store to row lo and runs the unwindowed kernels on the view (equal to
    them bit for bit, tests/test_gpu_sliding_window.py): here only the probes at the view's edges, with and (VALU hd32)
    without the new token."""
    _, knobs, kernel, _ = DECODE_ROUTES[route]
    for key, val in knobs.items():
        tunable(key, val)
    qplanes = kernel.startswith("decode_attn_partial_mfma_k<8") or kernel.startswith("decode_attn_lds")
    for c in host_window_cases(route):

        def log_ok(log):
            assert log[0].startswith(kernel.split("<")[0]), (route, log)
        _twice(K, c, "attn", log_ok, qplanes, route)


def test_large_slice_window_step(K):
    """A windowed kvq_decode_step with B * Hkv * D > 65,536: the new token is quantised by the regular quantise launches
    after the attention (not by the merge launch; the kernel log shows them). The attention is within budget, and slot T
    holds the unwindowed step's bytes."""
    B, Hq, Hkv, T, D, W = 72, 8, 8, 200, 128, 64
    assert B * Hkv * D > 65536
    c = A.make_case("probe", "decode", B, Hq, Hkv, T, 1, D, KINDS, "f16", seed=11, splits=(128,), probe_every=8, window=W)
    got, slots = [], []
    for poison, window in (("nan", W), ("huge", W), ("nan", 0)):  # the unwindowed step needs the whole store
        stores = device_stores(K, c, T + 3, POISON[poison], hide=c.lo if window else None)
        g, log, _ = run_case(K, c, "step", window=window, stores=stores)
        # partial, merge, then the K and the V quantise calls (at least one launch each)
        assert "merge" in log[1] and len(log) >= 4 and all(n.startswith(("quant", "absmax")) for n in log[2:]), log
        got.append(g)
        slots.append(stores.slot(T))
    for g in got[:2]:
        _check(c, g, True, "large-slice windowed step")
    assert np.array_equal(got[0], got[1])
    for s in slots[:2]:
        assert all(np.array_equal(a, b) for a, b in zip(s, slots[2]))
