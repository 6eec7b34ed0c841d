"""The attention checks can fail: on every input family and shape class of tests/test_gpu_attn_adversarial.py and the
extend shapes of tests/test_gpu_extend_attn.py, a float64 attention with ONE deliberate mistake (a chunk mask shifted by
one, a stored token dropped at a tile or split edge, two tokens' K or V scales swapped, the wrong GQA head map, the last
chunk token or decode's new token left out) is rejected by the same check and error budget the GPU tests apply
(tests/attn_cases.py), by at least a factor of 2 (a wrong kernel's own rounding cannot hide it). The unperturbed exact
attention passes. The same holds for every windowed route and family of tests/test_gpu_sliding_window_adversarial.py,
where the perturbations add a row's lower edge moved by one either way, row 0's edge for every row (extend), the chunk's
lower edge ignored, and the drops and scale swaps at the view's first token, its tiles and its splits. The same holds for
every row and count of tests/test_gpu_decode_dev_routes.py (decode with the count in device memory), where the
perturbations add the merge's live splits counted with the bound's split size, the last live split dropped, the first
dead split's slots attended, stored slot 0 attended at count 0 and the new token attended twice. The same holds for
every (route, start pattern, window, family) of tests/test_gpu_padded_attn_adversarial.py (left-padded batches), where the
perturbations are those of ``attn_cases.padded_perturbations``: a start moved by one either way, row 0's or the next
row's start, the start indexed by kv head, the start or the window ignored, a row's live splits counted with the
unpadded split size, its last live split dropped, its first dead split attended, chunk tokens before the start seen,
and a row that sees no key not zero. Runs without a GPU;
`pytest -s` prints every perturbation x case with its err / budget ratio."""
import numpy as np
import pytest

from tests import attn_cases as A
from tests.attn_cases import DECODE_ROUTES, EXTEND_ROUTES, KINDS
from tests.test_gpu_attn_adversarial import FAMILIES
from tests.test_gpu_decode_dev_routes import ROUTES, route_case, route_cases, route_plan
from tests.test_gpu_extend_attn import EDGE_CASES
from tests.test_gpu_padded_attn_adversarial import (DEV_SPARE, EXT_S, PAD_EXT, ROUTE, pad_decode_case, pad_decode_cases,
                                                    pad_extend_case, pad_extend_cases, qplanes_of)
from tests.test_gpu_padded_attn_adversarial import route_plan as padded_route_plan
from tests.test_gpu_sliding_window_adversarial import (WIN_DEV, WIN_EXTEND, host_window_cases, win_dev_case, win_dev_cases,
                                                       win_extend_cases)

MARGIN = 2.0

# the shapes of tests/test_gpu_extend_attn.py's EDGE_CASES rows, (B, Hq, Hkv, T, S, D). Those GPU rows run Gaussian
# inputs under the standard tolerance AND the budget; here the same shapes carry the families' inputs, because on a
# nearly flat Gaussian softmax one dropped token or swapped scale moves the output by ~1/T, which no check of tolerance
# size can see (the reason for the families).
EXTEND_SHAPES = EDGE_CASES + [shape for shape, _ in EXTEND_ROUTES.values()]


def _report(c, what):
    ref = c.reference()
    bud = A.bound(c, ref, qplanes=what.startswith("decode MFMA"))
    ok, r = A.check(A.attend(c), ref, bud)
    assert ok, ("the exact attention fails its own budget", what, r)
    lines, weak = [], []
    for name, kw in A.perturbations(c):
        got = A.attend(c, **kw)
        if np.isfinite(got).all():
            got = A.widen(A.narrow(got, c.dtype), c.dtype)  # what a kernel would write
        _, ratio = A.check(got, ref, bud)
        lines.append(f"{name}: {ratio:.3g}")
        if not ratio >= MARGIN:
            weak.append((name, ratio))
    what += f" W={c.window} T={c.T}" if c.window else ""
    print(f"{what} {c.info['family']}{'/' + c.info['variant'] if c.info['variant'] else ''} x{c.info['factor']:g} {c.dtype}: "
          f"rejected {len(lines) - len(weak)} / {len(lines)}: " + "; ".join(lines))
    assert len(lines) >= 8 and not weak, (what, c.info["family"], c.dtype, weak)


def _families(kind):
    for fam, extra, bf16 in FAMILIES:
        for dtype in ("f16", "bf16") if bf16 else ("f16",):
            yield fam, extra, dtype
    if kind == "extend":
        yield "sink", {"variant": "chunk"}, "f16"


@pytest.mark.parametrize("route", list(DECODE_ROUTES))
def test_decode_checks_reject_perturbations(route):
    (B, Hq, Hkv, T, D), _, kernel, splits = DECODE_ROUTES[route]
    what = ("decode MFMA " if "mfma" in kernel else "decode VALU ") + route
    for fam, extra, dtype in _families("decode"):
        _report(A.make_case(fam, "decode", B, Hq, Hkv, T, 1, D, KINDS, dtype, seed=len(route) + D, splits=splits, **extra), what)


@pytest.mark.parametrize("shape", EXTEND_SHAPES)
def test_extend_checks_reject_perturbations(shape):
    B, Hq, Hkv, T, S, D = shape
    _, ns, per = A.extend_plan(B, Hq, Hkv, T, S)
    for fam, extra, dtype in _families("extend"):
        c = A.make_case(fam, "extend", B, Hq, Hkv, T, S, D, KINDS, dtype, seed=T + S, splits=(per * 64,) if ns > 1 else (),
                        **extra)
        _report(c, f"extend {shape} ({ns} splits)")


def test_extend_plan_restatement_reaches_the_cap_and_short_last_splits():
    """The shapes above hit what they claim: a split count set by the 64-split cap alone; at T = 64 k - 1 / 64 k a last
    split shorter than the others, at 64 k + 1 a last tile of one token."""
    # the cap is the only limit: 96 splits by tile count (at least two tiles each), 512 by the workgroup target
    assert A.extend_plan(1, 32, 2, 12288, 4) == (1, 64, 3)
    assert (192 + 1) // 2 > A.EXT_MAX_SPLIT and A.EXT_TARGET_WG // 2 > A.EXT_MAX_SPLIT
    for T, last in ((319, 1), (320, 1), (321, 2)):
        _, ns, per = A.extend_plan(1, 32, 8, T, 16)
        assert (ns, per) == (3, 2) and (T + 63) // 64 - per * (ns - 1) == last


@pytest.mark.parametrize("route", list(WIN_EXTEND))
def test_extend_window_checks_reject_perturbations(route):
    cases, ns = win_extend_cases(route)
    for c in cases:
        _report(c, f"extend window {route} ({ns} splits)")


@pytest.mark.parametrize("route", list(WIN_DEV))
def test_device_count_window_checks_reject_perturbations(route):
    """Every (W, count, family) the GPU test runs, except W = 2000 on the head_dim-256 VALU routes (the costliest float64
    model here; W = 2000 runs on every other route, these two routes at W = 40 and 700)."""
    what = ("decode MFMA " if "mfma" in WIN_DEV[route][2] or "lds" in WIN_DEV[route][2] else "decode VALU ") + route
    for args in win_dev_cases(route, widths=(40, 700) if WIN_DEV[route][0][3] == 256 else None):
        _report(win_dev_case(route, *args), what)


@pytest.mark.parametrize("route", list(DECODE_ROUTES))
def test_host_count_window_checks_reject_perturbations(route):
    what = ("decode MFMA " if "mfma" in DECODE_ROUTES[route][2] or "lds" in DECODE_ROUTES[route][2] else "decode VALU ") + route
    for c in host_window_cases(route):
        _report(c, what + ("" if c.kn is not None else " (no new token)"))


@pytest.mark.parametrize("name", list(ROUTES))
def test_device_count_checks_reject_perturbations(name):
    """every (count, family) a device-count route runs: the exact attention passes; the new token left out and every
    perturbation of ``attn_cases.dev_perturbations`` are rejected by MARGIN"""
    p = route_plan(name)
    qplanes = ROUTES[name][1][0] == "int8" and "mfma" in ROUTES[name][4]
    for t, fam in route_cases(name):
        c = route_case(name, t, fam)
        ref = c.reference()
        bud = A.bound(c, ref, qplanes=qplanes)
        ok, r = A.check(A.attend(c), ref, bud)
        assert ok, ("the exact attention fails its own budget", name, t, fam, r)
        lines, weak = [], []
        dev = A.dev_perturbations(c, p, t)
        # the token-level mistakes of attn_cases.perturbations have their own routes; here the new token's
        for what, kw in [x for x in A.perturbations(c) if x[0] == "new token left out"] + dev:
            got = A.attend(c, **kw)
            if np.isfinite(got).all():
                got = A.widen(A.narrow(got, c.dtype), c.dtype)
            _, ratio = A.check(got, ref, bud)
            lines.append(f"{what}: {ratio:.3g}")
            if not ratio >= MARGIN:
                weak.append((what, ratio))
        print(f"{name} count {t} (live {p.live(t)}) {fam}: rejected {len(lines) - len(weak)} / {len(lines)}: " + "; ".join(lines))
        assert dev and not weak, (name, t, fam, weak)


# serving shapes of the device-count path: (B, Hq, Hkv, D, k_bits, bound) -> (partial, merge, nsplit, tiles per wave)
SERVING = {
    (8, 32, 8, 128, 8, 3100): ("decode_attn_lds_mfma_k<8, 4, 64, true, 2, 4, 128, true>", "decode_attn_merge_fast_k<2, true>", 13, 4),
    (4, 32, 8, 128, 8, 8200): ("decode_attn_lds_mfma_k<8, 4, 64, true, 2, 4, 128, true>", "decode_attn_merge_fast_k<16, true>", 26, 5),
    (1, 32, 8, 128, 8, 32768): ("decode_attn_lds_mfma_k<8, 4, 64, true, 2, 4, 128, true>", "decode_attn_merge_fast_k<16, true>", 128, 4),
    (1, 8, 1, 128, 8, 40000): ("decode_attn_partial_mfma_k<8, 4, 128, 128, false>", "decode_attn_merge_k", 313, 0),
}


def test_device_count_plan_restatement():
    """``attn_cases.dev_plan`` gives every row of tests/test_gpu_decode_dev_routes.py the kernels, merge form and new-token
    routine the row states (the GPU test asserts the kernel log against the same names), and the serving shapes the plan
    the host takes for them: the ring past 16 splits at batch 4 with 8 K tokens and at batch 1 with 32 K, the chained
    merge past 256 one-tile splits"""
    for name, row in ROUTES.items():
        p = route_plan(name)
        assert (p.partial, p.merge, p.by_wave, p.append) == tuple(row[4:8]), (name, p)
    for (B, Hq, Hkv, D, kb, bound), want in SERVING.items():
        p = A.dev_plan(B, Hq, Hkv, D, kb, bound)
        assert (p.partial, p.merge, p.nsplit, p.tpw) == want, ((B, Hq, Hkv, D, kb, bound), p)
    # the live layout: ceil(tiles / nsplit) tiles per wave, the count clamped to the bound
    p = A.dev_plan(4, 32, 8, 128, 8, 8200)
    assert p.live(6656) == (256, 26) and p.live(6657) == (320, 21) and p.live(0) == (64, 0) and p.live(9000) == p.live(8200)
    assert A.dev_plan(1, 8, 1, 128, 8, 40000).live(32769) == (128, 257)
    assert A.dev_plan(1, 8, 2, 128, 8, 2600, {"attn_ring_dev": 0}).partial.startswith("decode_attn_partial_mfma_k<")


def _dead_rows(c):
    """[B, S] (decode: [B]): the rows that see no key, from the case's starts, the rows' positions and the window"""
    ext = c.mode == "extend"
    pos = c.T + np.arange(c.S) if ext else np.array([c.T - (c.kn is None)])
    lo = np.maximum(np.asarray(c.kv_start)[:, None], (pos + 1 - c.window if c.window else 0 * pos)[None, :])
    dead = lo > pos[None, :]
    return dead if ext else dead[:, 0]


def _live_ratio(got, ref, bud):
    """worst err / budget over the elements of rows that see a key (budget > 0)"""
    if not np.isfinite(got).all():
        return float("inf")
    live = bud > 0
    return float((np.abs(got - ref)[live] / bud[live]).max()) if live.any() else 0.0


def _report_padded(c, plan, what, qplanes):
    """The exact attention passes; every padded perturbation is rejected by MARGIN. A mistake in the start or the window
    (``starts=`` / ``wignore=`` of ``attend``) is judged PER BATCH ROW and on the rows' live elements alone: every batch
    row that sees a key and whose first visible key the mistake moves must reject it by itself, and the figure printed
    is the weakest such row's. The start indexed by kv head is the exception: it moves single (row, kv head) pairs, up or
    down, and with two kv heads a pair carries the row's "in" or its "out" probe, not both; there the best moved row
    counts, still on live elements alone. (A row that sees no key has budget 0, so any non-zero output there is an
    infinite ratio that would hide whether the other rows' probes notice; where ONLY such rows are moved the whole
    tensor is judged.)
    Returns the perturbations' names."""
    ref = c.reference()
    bud = A.bound(c, ref, qplanes=qplanes)
    ok, r = A.check(A.attend(c), ref, bud)
    assert ok, ("the exact attention fails its own budget", what, r)
    dead = np.broadcast_to(np.expand_dims(_dead_rows(c), 1), ref.shape[:-1])  # over the query heads
    assert np.array_equal(bud.max(axis=-1) == 0, dead), (what, "the rows of budget 0 are not the rows that see no key")
    assert (ref[dead] == 0).all(), (what, "a row that sees no key is not zero in the reference")
    first = A.padded_first(c)
    live_b = [bool((bud[b] > 0).any()) for b in range(c.B)]
    lines, weak = [], []
    for name, kw in A.padded_perturbations(c, plan):
        got = A.attend(c, **kw)
        if np.isfinite(got).all():
            got = A.widen(A.narrow(got, c.dtype), c.dtype)  # what a kernel would write
        moved = []
        if "starts" in kw or "wignore" in kw:
            now = A.padded_first(c, kw.get("starts"), kw.get("wignore", False))
            moved = [b for b in range(c.B) if live_b[b] and not np.array_equal(now[b], first[b])]
        if moved:  # the kv-head index is one mistake of the whole launch, and moves single (row, kv head) pairs either way
            ratio = (max if "kv head" in name else min)(_live_ratio(got[b], ref[b], bud[b]) for b in moved)
        else:
            _, ratio = A.check(got, ref, bud)
        lines.append(f"{name}: {ratio:.3g}")
        if not ratio >= MARGIN:
            weak.append((name, ratio))
    print(f"{what} {c.info['family']}{'/' + c.info['variant'] if c.info['variant'] else ''} {c.dtype}: "
          f"rejected {len(lines) - len(weak)} / {len(lines)}: " + "; ".join(lines))
    assert lines and not weak, (what, c.info["family"], c.dtype, weak)
    return [x.split(":")[0] for x in lines]


def _start_probes(c, hi):
    """each batch row with 0 < start_b < hi carries at least one "in" and one "out" start probe"""
    for b, s in enumerate(c.kv_start):
        if 0 < s < hi:
            n = c.info["start_probes"][b]
            assert n["in"] >= 1 and n["out"] >= 1, (b, c.kv_start, n)


@pytest.mark.parametrize("name", list(ROUTE))
def test_padded_decode_checks_reject_perturbations(name):
    """Every (start pattern, window, family) of a padded decode route; the route's cases together apply every mistake of
    ``attn_cases.padded_perturbations`` that the route's layout can make."""
    (B, Hq, Hkv, D), T = ROUTE[name][:2]
    names = set()
    for args in pad_decode_cases(name):
        pat, starts, W, with_new = args[:4]
        c, plan = pad_decode_case(name, *args)
        # the Python restatement of the per-row layout agrees with the plan's, and the device-count step under the bound
        # T + DEV_SPARE has the launch's layout
        dev = padded_route_plan(name, W, with_new, spare=DEV_SPARE)
        assert (dev.ts, dev.nsplit, dev.tpw) == (plan.ts, plan.nsplit, plan.tpw), (name, W, plan, dev)
        for lo in c.los:
            assert A.padded_live(plan, T - lo) == plan.live(T - lo) == dev.live(T - lo), (name, lo)
        _start_probes(c, T)
        if W:  # the window wins for some rows, the start for others
            assert any(lo == c.lo for lo in c.los) and any(lo > c.lo for lo in c.los), (name, starts, W, c.los)
        names |= set(_report_padded(c, plan, f"padded {name} {pat} starts={starts} W={W}" + ("" if with_new else " (no new token)"),
                                    qplanes_of(name, plan.partial)))
    plan = padded_route_plan(name)
    want = ["start edge +1", "start edge -1", "row 0's start", "row (b + 1) % B's start", "start ignored under the window",
            "window ignored where a start is set", "a row that sees no key is not zero"]
    want += ["start indexed by kv head"] if Hkv > 1 else []
    want += ["last live split dropped", "first dead split attended"] if plan.nsplit > 1 else []
    want += ["live splits counted with the unpadded split size"] if plan.tpw else []
    missing = [w for w in want if not any(n.startswith(w) for n in names)]
    assert not missing, (name, missing, sorted(names))
    if plan.tpw:  # the rows of the split pattern differ in tiles per wave and in live split count
        pat, starts = next((a[0], a[1]) for a in pad_decode_cases(name) if a[0] == "split" and a[2] == 0)
        lay = {A.padded_live(plan, T - s) for s in starts}
        assert len({ts for ts, _ in lay}) > 1 and len({ns for _, ns in lay}) > 1, (name, starts, lay)


@pytest.mark.parametrize("S", EXT_S)
@pytest.mark.parametrize("shape", PAD_EXT, ids=[f"B{s[0]}-Hq{s[1]}-Hkv{s[2]}-T{s[3]}-D{s[4]}" for s in PAD_EXT])
def test_padded_extend_checks_reject_perturbations(shape, S):
    B, _, Hkv, T = shape[:4]
    names = set()
    for starts, W, fam, extra in pad_extend_cases(shape, S):
        c, ns = pad_extend_case(shape, S, starts, W, fam, extra)
        _start_probes(c, T + S)
        names |= set(_report_padded(c, None, f"padded extend {shape[:5]} S={S} ({ns} splits) starts={starts} W={W}", False))
    want = ["start edge +1", "start edge -1", "row 0's start", "row (b + 1) % B's start", "padding rows given their own token's V",
            "start ignored under the window"]
    # T = 0: no row can have 0 < start < T + S - W at S = 1, and at S = 40 / 130 the cases' W = S // 2 puts the window's
    # last bound, S - W, at or below the padded row's start
    want += ["window ignored where a start is set"] if T else []
    want += ["start indexed by kv head"] if B > 1 and Hkv > 1 else []
    want += ["chunk tokens before the start seen by later rows"] if S > 1 else []
    missing = [w for w in want if not any(n.startswith(w) for n in names)]
    assert not missing, (shape, S, missing, sorted(names))


def test_padded_extend_shapes_launch_one_split_and_several():
    """the padded extend cases run the one-split form and the split form with extend_attn_merge_padded_k, at every S"""
    for S in EXT_S:
        seen = {A.extend_plan(*shape[:3], shape[3] - A.view_lo("extend", shape[3], W), S)[1] > 1
                for shape in PAD_EXT for _, W, _, _ in pad_extend_cases(shape, S)}
        assert seen == {False, True}, (S, seen)
