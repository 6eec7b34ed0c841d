"""Left-padded attention (``kv_start``, the kvq_*_padded entry points) on adversarial inputs (tests/attn_cases.py with
``kv_start=``): every padded route of tests/test_gpu_padded_attn.py::ROUTES and the padded extend are checked against the
float64 model of tests/attn_ref.py under the per-element budget of ``attn_cases.bound``, on cases whose positional
probes sit at EVERY batch row's own key start (a target at lo_b the row must see, one at lo_b - 1 it must not), at
lo_b + 63 / 64, at T - 1 and on both sides of the boundaries of the row's own split layout (the ring spreads row b's live
tiles by its own count, ``attn_cases.padded_live``). tests/test_attn_discrimination.py shows that the same check rejects a
start moved by one, another row's start, a start indexed by kv head, a start or a window ignored, a live split count
taken from the unpadded layout, a dropped last split and an attended dead one.

Start patterns per route (every one with a row at start 0, the row that needs every slot's scale): the live counts of
three rows one below, at and one above a multiple of the row split size (the ring: nsplit * 64, where a row's tiles per
wave and live split count change), rows whose lo_b is 63, 64 and 65 mod 64, and, without the new token, a row at T that
sees nothing and must be exactly zero. Each runs with W = 0 and with a W whose bound lies between the rows' starts (the
window wins for some rows, the start for others), one family per (pattern, W) in turn.

Every case runs on three stores whose outputs must be bit-identical: "decoy" (the padding slots hold the case's own
quantised tokens, the forbidden targets among them), "nan" (row b's slots before lo_b hold extreme codes, the scale slots
no row needs NaN) and "huge" (the same with scales of 1e30: ``fmaxf`` drops a NaN, so a poisoned scale folded into a
running V-scale maximum passes the NaN run)."""
import numpy as np
import pytest

from tests import attn_cases as A
from tests.attn_cases import BITS
from tests.gpu_harness import K, device_stores, run_case, tunable  # noqa: F401
from tests.test_gpu_padded_attn import EXT, ROUTES
from tests.util import to_torch

pytestmark = pytest.mark.gpu

POISON = {"decoy": None, "nan": float("nan"), "huge": 1e30}
FAMILIES = [("probe", {}), ("sink", {}), ("sink", {"variant": "lo"}), ("late", {}), ("vrange", {})]
ROUTE = {r[0]: r[1:] for r in ROUTES}
DEV_SPARE = 3  # the device-count step runs at count T under the bound T + 3


def route_plan(name, W=0, with_new=True, spare=0):
    (B, Hq, Hkv, D), T, kinds, tun = ROUTE[name][:4]
    return A.padded_plan(B, Hq, Hkv, D, BITS[kinds[0]], T + spare, W, with_new, tun, v_bits=BITS[kinds[1]])


def start_patterns(name):
    """(pattern name, starts [B], with the new token) of a route; see the module docstring"""
    (B, _, _, _), T = ROUTE[name][:2]
    p = route_plan(name)
    step = p.nsplit * 64 if p.tpw else p.ts  # a row's layout changes where its live count passes a multiple of this
    if step >= T:
        step = 64
    m = max(1, T // step // 2) * step
    below, at, above = T - (m - 1), T - m, T - (m + 1)  # live counts m - 1, m, m + 1
    a = 64 * max(1, T // 64 // 3)
    if B >= 4:
        pats = [("split", [0, below, at, above]), ("tile", [a + 63, 0, a + 64, a + 65])]
    else:
        pats = [("split", [0, below, above]), ("split'", [at, 0, a + 64]), ("tile", [a + 63, a + 65, 0])]
    out = [(n, s + [0] * (B - len(s)), True) for n, s in pats]
    out.append(("dead row", ([T, 0, below] + [a + 64] * B)[:B], False))
    return out


def window_for(starts, T):
    """a window whose bound (with the new token) lies between the smallest and the largest start in (0, T)"""
    mid = sorted(s for s in starts if 0 < s < T)
    return T + 1 - (mid[0] + mid[-1] + 1) // 2


def pad_decode_cases(name):
    """(pattern, starts, W, with_new, family, make_case keyword arguments, dtype): every pattern with both windows, one
    family per (pattern, W) in turn"""
    T = ROUTE[name][1]
    i = len(name)
    for pat, starts, with_new in start_patterns(name):
        for W in (0, window_for(starts, T)):
            fam, extra = FAMILIES[i % len(FAMILIES)]
            yield pat, starts, W, with_new, fam, extra, ("f16", "bf16")[i % 2]
            i += 1


def pad_decode_case(name, pat, starts, W, with_new, fam, extra, dtype):
    """the case and the plan of its launches (host count T; the device-count step's bound T + 3 plans the same layout)"""
    (B, Hq, Hkv, D), T, kinds, _ = ROUTE[name][:4]
    plan = route_plan(name, W, with_new)
    los = A.padded_los("decode", T, W, with_new, A.clamp_starts("decode", starts, T, 1))
    splits = [(A.padded_live(plan, T - lo)[0],) for lo in los]
    c = A.make_case(fam, "decode", B, Hq, Hkv, T, 1, D, kinds, dtype, seed=T + W + len(pat), splits=splits, with_new=with_new,
                    window=W, kv_start=starts, **extra)
    return c, plan


def qplanes_of(name, partial):
    """the int8 query planes' term of the budget: INT8 keys on the MFMA or ring kernels. ``partial``: the kernel of the
    launch itself (the kernel log's, or the plan's for the case's own window: a window plans for fewer tokens and may
    take another family than the route's)."""
    return ROUTE[name][2][0] == "int8" and "mfma" in partial


# extend: EXT's shapes; the last with a store of 60 tokens (one split with a store; T = 0 is one split without one)
PAD_EXT = [EXT[0], EXT[1], EXT[2], EXT[3][:3] + (60,) + EXT[3][4:]]
EXT_S = (1, 40, 130)


def pad_extend_cases(shape, S):
    """(starts, W, family, keyword arguments): starts inside the store, at T and reaching into the chunk, each with W = 0
    and a W whose bound overtakes the inner start in the middle of the chunk"""
    B, Hq, Hkv, T, D = shape[:5]
    inner = T // 2 // 64 * 64 + 63 if T >= 128 else T // 2
    i = T + S
    for starts in ([0, inner, T + (S + 1) // 2], [T, 0, T + max(S - 1, 1)]):
        for W in (0, max(1, T - starts[1 if starts[0] == 0 else 0] + S // 2)):
            fam, extra = FAMILIES[i % len(FAMILIES)]
            yield starts, W, fam, extra
            i += 1


def pad_extend_case(shape, S, starts, W, fam, extra):
    """the case and the split count of its launch (planned over the window's view [lo0, T))"""
    B, Hq, Hkv, T, D, kinds, dtype = shape
    lo0 = A.view_lo("extend", T, W)
    _, ns, per = A.extend_plan(B, Hq, Hkv, T - lo0, S)
    c = A.make_case(fam, "extend", B, Hq, Hkv, T, S, D, kinds, dtype, seed=T + S + W, splits=(per * 64,) if ns > 1 else (),
                    window=W, kv_start=starts, **extra)
    return c, ns


def _stores(K, c, cap, store):
    """Device stores of cap slots. "decoy": every slot below T holds the case's own codes and scales. "nan" / "huge": row
    b's slots before lo_b hold extreme codes and the scale slots below min_b lo_b the poison. Slots from T on: extreme
    codes and a poison scale in every store."""
    if POISON[store] is None:
        return device_stores(K, c, cap, 1e30)
    return device_stores(K, c, cap, POISON[store], hide=c.los)


def _judge(c, outs, ref, bud, what, worst):
    """every store's output within the budget, rows that see no key exactly zero, the stores bit-identical"""
    dead = np.abs(bud).max(axis=-1) == 0
    for store, got in outs.items():
        ok, r = A.check(got, ref, bud)
        worst[0] = max(worst[0], r)
        assert ok, (what, store, c.info["family"], c.info["variant"], c.dtype, c.kv_start, c.window, r)
        assert (got[dead] == 0).all(), (what, store, "a row that sees no key is not zero")
    first = next(iter(outs.values()))
    for store, got in outs.items():
        assert np.array_equal(got, first), (what, store, c.kv_start, c.window, "the stores' outputs differ")


DECODE_CASES = [(name, i) for name in ROUTE for i in range(len(list(pad_decode_cases(name))))]


@pytest.mark.parametrize("name,index", DECODE_CASES, ids=[f"{n}-{i}" for n, i in DECODE_CASES])
def test_padded_decode_on_adversarial_inputs(K, tunable, name, index):
    """kvq_decode_attn_padded (with the new token; the "dead row" pattern without it) and kvq_decode_step_dev_padded at
    count T below the bound T + 3, on one (start pattern, window) of the route."""
    (B, Hq, Hkv, D), T, kinds, tun, partial, merge = ROUTE[name]
    for key, val in tun.items():
        tunable(key, val)
    worst = [0.0]
    for args in list(pad_decode_cases(name))[index:index + 1]:
        pat, starts, W, with_new, fam, extra, dtype = args
        c, plan = pad_decode_case(name, *args)
        ref = c.reference()
        bud = None
        host, dev = {}, {}
        for store in POISON:
            stores = _stores(K, c, T + DEV_SPARE + 2, store)
            host[store], log, _ = run_case(K, c, "attn", kv_start=starts, stores=stores)
            if W == 0:  # the planned route (a window plans for fewer tokens and may take another)
                assert log[0] == partial and log[1].startswith(merge), (name, log)
            assert log and all("_padded_k" in n for n in log), (name, log)
            # the kernel family the CPU proof (tests/test_attn_discrimination.py) budgets this case for
            assert ("mfma" in log[0]) == ("mfma" in plan.partial), (name, W, log, plan)
            if bud is None:
                bud = A.bound(c, ref, qplanes=qplanes_of(name, log[0]))
            if with_new:  # the device-count step: the store has spare slots, the count equals T
                dev[store], dlog, _ = run_case(K, c, "dev", kv_start=starts, bound=T + DEV_SPARE, stores=stores)
                assert all("_padded_k" in n for n in dlog) and ("mfma" in dlog[0]) == ("mfma" in log[0]), (name, W, dlog, log)
        what = f"{name} {pat} starts={starts} W={W} {fam}"
        _judge(c, host, ref, bud, what + " host count", worst)
        if with_new:
            _judge(c, dev, ref, bud, what + " device count", worst)
        print(f"padded decode [{name}] {pat} W={W} {fam} {dtype}: worst err / budget {worst[0]:.3f}")


@pytest.mark.parametrize("S", EXT_S)
@pytest.mark.parametrize("shape", PAD_EXT, ids=[f"B{s[0]}-Hq{s[1]}-Hkv{s[2]}-T{s[3]}-D{s[4]}" for s in PAD_EXT])
def test_padded_extend_on_adversarial_inputs(K, shape, S):
    """kvq_extend_attn_padded: one split (T = 0, T = 60) and several plus extend_attn_merge_padded_k; the chunk's padded
    prefix is poisoned too (k_new NaN, v_new inf) on the "nan" and "huge" stores."""
    B, Hq, Hkv, T, D, kinds, dtype = shape
    dt = {"f16": 0, "bf16": 1}[dtype]
    worst = [0.0]
    for starts, W, fam, extra in pad_extend_cases(shape, S):
        c, ns = pad_extend_case(shape, S, starts, W, fam, extra)
        ref = c.reference()
        bud = A.bound(c, ref)
        outs = {}
        for store in POISON:
            kn, vn = to_torch(c.kn, dtype), to_torch(c.vn, dtype)
            if POISON[store] is not None:
                for b, s in enumerate(c.kv_start):  # the chunk's padded prefix
                    if s > T:
                        kn[b, :, :s - T] = float("nan")
                        vn[b, :, :s - T] = float("inf")
            outs[store], log, _ = run_case(K, c, "extend", kv_start=starts, stores=_stores(K, c, T + 3, store), kn=kn, vn=vn)
            assert log[0] == f"extend_attn_padded_k<{BITS[kinds[0]]}, {BITS[kinds[1]]}, {D}, {dt}>" and \
                log[1:] == ([f"extend_attn_merge_padded_k<{D}, {dt}>"] if ns > 1 else []), (shape, S, starts, W, ns, log)
        _judge(c, outs, ref, bud, f"extend {shape[:5]} S={S} starts={starts} W={W} {fam}", worst)
    print(f"padded extend {shape[:5]} S={S}: worst err / budget {worst[0]:.3f}")
