"""Decode with the stored-token count in device memory (kvq_decode_step_dev: what a captured decode graph replays) through
every (partial, merge, new-token append) combination it can take, on adversarial inputs (tests/attn_cases.py) whose
probes sit on the LIVE split edges of each count.

The host plans the launch from an upper bound; the kernels derive the rest from the count: the ring kernel's tiles per
wave (ring_dev_tpw), the merge's split size and live split count (live_split_tokens), the new token's slot. Every row of
ROUTES states its shape, bound and tunables and the kernels it runs; ``attn_cases.dev_plan`` (a restatement of the host's
plan) must predict them (tests/test_attn_discrimination.py, on the CPU) and the kernel log must show them. The count is
swept over 0, 1, the first tile edges, both sides of the counts where the live layout changes, the bound and past it
(clamped: bit-identical to the bound). Each (row, count) takes one family in turn.

Every call is checked against the float64 oracle under ``attn_cases.bound``; the slot at the count must hold the oracle's
quantised new token and nothing else may change, guard slots before and after the store included. Every call runs twice,
and the two must be bit-identical: once with the workspace full of NaN and the store slots past the count holding extreme
codes with NaN scales; once with the workspace a call at the bound left behind on a store whose every token is a sink (a
dominant ``m`` in every split row, the dead ones of a smaller count included: ``fmaxf`` drops a NaN, so the NaN run alone
would pass a merge that reads dead rows) and the slots past the count holding extreme codes with scales of 1e30.

The rows are the smallest shapes that reach each route: the kernels see only the split layout (nsplit, split size) and
the count, and where a serving shape would take the ring by size, ``attn_stream_tpw`` sets the same layout at a batch the
float64 model can afford. tests/test_attn_discrimination.py::test_device_count_plan_restatement pins the plan of the
serving shapes themselves (the ring past 16 splits at batch 4 with 8 K tokens, the chained merge past 32 K tokens)."""
import copy

import numpy as np
import pytest
import torch

from oracle import kvq_oracle as O
from tests import attn_cases as A
from tests.attn_cases import BITS
from tests.attn_cases import KINDS as I8I4
from tests.gpu_harness import POISON, K, device_stores, got64, tunable  # noqa: F401
from tests.util import to_numpy, to_torch

pytestmark = pytest.mark.gpu

# name -> (B, Hq, Hkv, D), kinds, bound, tunables, partial (kernel-log prefix), merge, merge by one wave per head, append
ROUTES = {
    "ring hd128 TG4, <2, true> by wave": (
        (1, 8, 2, 128), I8I4, 1900, {"attn_stream_tpw": 2},
        "decode_attn_lds_mfma_k<8, 4, 64, true, 2, 4, 128, true>", "decode_attn_merge_fast_k<2, true>", True, "regs"),
    "ring hd128 TG4, <16, true>": (
        (1, 8, 2, 128), I8I4, 2600, {"attn_stream_tpw": 2},
        "decode_attn_lds_mfma_k<8, 4, 64, true, 2, 4, 128, true>", "decode_attn_merge_fast_k<16, true>", False, "regs"),
    "ring hd128 TG1, <16, true>": (
        (1, 16, 2, 128), I8I4, 3300, {"attn_stream_tpw": 3},
        "decode_attn_lds_mfma_k<8, 4, 64, true, 2, 1, 128, true>", "decode_attn_merge_fast_k<16, true>", False, "regs"),
    "ring hd128 INT4 keys, <16, true>": (
        (1, 8, 2, 128), ("int4", "int8"), 2600, {"attn_stream_tpw": 2},
        "decode_attn_lds_mfma_k<4, 8, 64, false, 2, 1, 128, true>", "decode_attn_merge_fast_k<16, true>", False, "regs"),
    "ring hd64 TG4, <2, true> workgroups": (
        (1, 8, 2, 64), I8I4, 2600, {"attn_stream_tpw": 2},
        "decode_attn_lds_mfma_k<8, 4, 64, true, 2, 4, 64, true>", "decode_attn_merge_fast_k<2, true>", False, "regs"),
    "ring hd64 TG1, <2, true> workgroups": (
        (1, 16, 2, 64), ("int8", "int8"), 3300, {"attn_stream_tpw": 3},
        "decode_attn_lds_mfma_k<8, 8, 64, true, 2, 1, 64, true>", "decode_attn_merge_fast_k<2, true>", False, "regs"),
    "ring hd64, <16, true>": (
        (1, 8, 2, 64), I8I4, 4400, {"attn_stream_tpw": 2},
        "decode_attn_lds_mfma_k<8, 4, 64, true, 2, 4, 64, true>", "decode_attn_merge_fast_k<16, true>", False, "regs"),
    "ring hd128, attn_merge_wave 0: <2, true> workgroups": (
        (1, 8, 2, 128), I8I4, 1900, {"attn_stream_tpw": 2, "attn_merge_wave": 0},
        "decode_attn_lds_mfma_k<8, 4, 64, true, 2, 4, 128, true>", "decode_attn_merge_fast_k<2, true>", False, "regs"),
    "ring hd128, attn_merge_fast 0: chained merge": (
        (1, 8, 2, 128), I8I4, 2600, {"attn_stream_tpw": 2, "attn_merge_fast": 0},
        "decode_attn_lds_mfma_k<8, 4, 64, true, 2, 4, 128, true>", "decode_attn_merge_k", False, "block"),
    "one-tile MFMA, <2, false> by wave": (
        (1, 8, 2, 128), I8I4, 1500, {},
        "decode_attn_partial_mfma_k<8, 4, 128, 128, false>", "decode_attn_merge_fast_k<2, false>", True, "regs"),
    "one-tile MFMA, <16, false>": (
        (1, 8, 2, 128), I8I4, 3000, {},
        "decode_attn_partial_mfma_k<8, 4, 128, 128, false>", "decode_attn_merge_fast_k<16, false>", False, "regs"),
    "one-tile MFMA, 257 splits: chained merge": (
        (1, 2, 1, 128), I8I4, 32769, {},
        "decode_attn_partial_mfma_k<8, 4, 128, 128, false>", "decode_attn_merge_k", False, "block"),
    "VALU hd32": (
        (1, 8, 2, 32), I8I4, 3000, {},
        "decode_attn_partial_k<8, 4, 4>", "decode_attn_merge_fast_k<2, false>", False, "regs"),
    "VALU hd256, <16, false>": (
        (1, 8, 2, 256), I8I4, 1100, {},
        "decode_attn_partial_k<8, 4, 4>", "decode_attn_merge_fast_k<16, false>", False, "regs"),
    "VALU forced at hd128": (
        (1, 16, 2, 128), I8I4, 2000, {"attn_force_valu": 1},
        "decode_attn_partial_k<8, 4, 8>", "decode_attn_merge_fast_k<2, false>", True, "regs"),
    "append by pieces beside a ring merge": (
        (17, 4, 4, 128), I8I4, 260, {"attn_stream_tpw": 2},
        "decode_attn_lds_mfma_k<8, 4, 64, true, 2, 4, 128, true>", "decode_attn_merge_fast_k<2, true>", True, "parts"),
    "append by one workgroup beside a ring merge": (
        (17, 4, 4, 128), I8I4, 260, {"attn_stream_tpw": 2, "attn_new_token_parts": 0},
        "decode_attn_lds_mfma_k<8, 4, 64, true, 2, 4, 128, true>", "decode_attn_merge_fast_k<2, true>", True, "block"),
}
FAMILIES = ["probe", "sink", "late", "vrange"]
GUARD = 3       # guard slots before and after each store
WS_GUARD = 256  # guard floats behind the workspace the plan needs
SENTINEL = 12345.0


def route_plan(name):
    (B, Hq, Hkv, D), kinds, bound, knobs = ROUTES[name][:4]
    return A.dev_plan(B, Hq, Hkv, D, BITS[kinds[0]], bound, knobs, v_bits=BITS[kinds[1]])


def route_counts(name):
    """the counts a row sweeps: 0, 1, the first tile edges, both sides of the first change of the ring's tiles per wave
    and of the last change of the live layout, bound - 1, bound, bound + 5"""
    p = route_plan(name)
    ch = A.dev_plan_changes(p)
    tpw_ch = [t for t in ch if p.live(t)[0] != p.live(t - 1)[0]]
    picks = set(tpw_ch[:1]) | set(list(ch)[-1:])
    counts = {0, 1, 63, 64, 65, 127, 128, 129, p.bound - 1, p.bound} | picks | {t - 1 for t in picks}
    return sorted(t for t in counts if t <= p.bound) + [p.bound + 5]


def route_cases(name):
    """(count, family) of a row, one family per count in turn (count 0: ``probe``; bound + 5 reuses the bound's case)"""
    out = []
    for i, t in enumerate(route_counts(name)[:-1]):
        out.append((t, "probe" if t == 0 else FAMILIES[i % len(FAMILIES)]))
    return out


def route_case(name, t, fam):
    """the case of (row, count): probes on the new token, on the last stored token and on both sides of the last live
    split's first token first, then on tokens 0, 63, 64 and the first live split edge (at least four probe rows)"""
    (B, Hq, Hkv, D), kinds = ROUTES[name][:2]
    ts, ns = route_plan(name).live(t)
    last = (ns - 1) * ts
    return A.make_case(fam, "decode", B, Hq, Hkv, t, 1, D, kinds, "f16", seed=t + D + len(name), splits=(ts,),
                       probe_every=max(1, B * Hq // 4), targets=(t - 1, last - 1, last, 0, 63, 64, ts - 1, ts))


def _new_token_codes(c):
    """the oracle's quantised new token: (K codes [B,Hkv,Dq], K scale, V codes, V scale)"""
    out = []
    for x, kind in ((c.kn, c.kinds[0]), (c.vn, c.kinds[1])):
        q, _, s = O.quantize_tokens(x[None, :, :, None, :], kind)
        out += [q[0][:, :, 0], s[0, 0]]
    return out


class Stores:
    """tests/gpu_harness.py::device_stores of ``cap`` slots with GUARD slots on each side (slots [0, T) hold the case's codes
    and scales; every other slot, the guards included, extreme codes and the poison scale), and what they first held."""

    def __init__(self, K, c, cap, poison):
        st = device_stores(K, c, cap, POISON[poison], guard=GUARD)
        self.bufs, self.views = st.bufs, st.views
        self.before = [b.clone() for b in self.bufs]

    def expected(self, slot, codes):
        """the buffers as the step must leave them: ``codes`` (of _new_token_codes) in ``slot``, nothing else changed"""
        exp = [b.clone() for b in self.before]
        for i in (0, 2):
            exp[i][:, :, GUARD + slot] = to_torch(np.ascontiguousarray(codes[i]))
            exp[i + 1][GUARD + slot] = float(codes[i + 1])
        return exp


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _stale_workspace(K, name, ws_len):
    """the workspace a call at the bound leaves behind on a store whose every slot holds one sink token (tests/attn_cases.py,
    family ``sink``: 12-20 nats above the rest for all but one query row): every split row of every head holds a
    dominant ``m``"""
    (B, Hq, Hkv, D), kinds, bound = ROUTES[name][:3]
    c = A.make_case("sink", "decode", B, Hq, Hkv, 1, 1, D, kinds, "f16", seed=3, probe_every=10 ** 9)
    cap = bound + 8
    k_store = to_torch(c.kq).expand(B, Hkv, cap, c.kq.shape[-1]).contiguous()
    v_store = to_torch(c.vq).expand(B, Hkv, cap, c.vq.shape[-1]).contiguous()
    k_sc = torch.full((cap,), float(c.ks[0]), device="cuda")
    v_sc = torch.full((cap,), float(c.vs[0]), device="cuda")
    q = to_torch(np.ascontiguousarray(c.q[:, :, 0]), "f16")
    ws = torch.full((ws_len,), float("nan"), device="cuda")
    plan = K.DecodeStepPlan(q, k_store, k_sc, kinds[0], v_store, v_sc, kinds[1], 1e-8)
    t_dev = torch.full((1,), bound, dtype=torch.int32, device="cuda")
    K.decode_step_dev(plan, q, to_torch(c.kn, "f16"), to_torch(c.vn, "f16"), t_dev, bound, torch.empty_like(q), ws, c.sm)
    torch.cuda.synchronize()
    return ws


@pytest.mark.parametrize("name", list(ROUTES))
def test_device_count_route(K, tunable, name):
    from efficient_llm_inference_amd import _lib
    (B, Hq, Hkv, D), kinds, bound, knobs, partial, merge = ROUTES[name][:6]
    for key, val in knobs.items():
        tunable(key, val)
    p = route_plan(name)
    assert (p.partial, p.merge) == (partial, merge), (name, p)
    cap = bound + 8
    need = K.decode_attn_workspace(B, Hq, Hkv, bound, D)
    stale = _stale_workspace(K, name, need + WS_GUARD)
    stale[need:] = SENTINEL
    qplanes = kinds[0] == "int8" and "mfma" in partial
    at_bound = None
    for t, fam in route_cases(name) + [(bound + 5, None)]:
        if fam:
            c = route_case(name, t, fam)
            ref = c.reference()
            bud = A.bound(c, ref, qplanes=qplanes)
        slot = min(t, bound)  # bound + 5: the bound's case, clamped
        codes = _new_token_codes(c)
        res = []
        for ws_kind, poison in (("nan", "nan"), ("stale", "huge")):
            st = Stores(K, c, cap, poison)
            q = to_torch(np.ascontiguousarray(c.q[:, :, 0]), "f16")
            vn = to_torch(c.vn, "f16")
            out = torch.full(q.shape, float("nan"), dtype=torch.float16, device="cuda")
            if ws_kind == "nan":
                ws = torch.full((need + WS_GUARD,), float("nan"), device="cuda")
                ws[need:] = SENTINEL
            else:
                ws = stale.clone()
            plan = K.DecodeStepPlan(q, st.views[0], st.views[1], kinds[0], st.views[2], st.views[3], kinds[1], 1e-8)
            t_dev = torch.full((1,), t, dtype=torch.int32, device="cuda")
            _lib.kernel_log_clear()
            K.decode_step_dev(plan, q, to_torch(c.kn, "f16"), vn, t_dev, bound, out, ws, c.sm)
            torch.cuda.synchronize()
            log = _lib.kernel_log()
            assert log == [partial, merge], (name, t, log)
            ok, r = A.check(got64(out), ref, bud)
            assert ok, (name, t, fam, ws_kind, poison, r)
            if t == 0:  # one softmax term of weight exactly 1: v_new itself
                assert torch.equal(out.view(torch.int16), vn.repeat_interleave(Hq // Hkv, dim=1).view(torch.int16)), name
            for a, e, what in zip(st.bufs, st.expected(slot, codes), ("K codes", "K scales", "V codes", "V scales")):
                assert torch.equal(_bits(a), _bits(e)), (name, t, what, "slot", slot)
            assert bool((ws[need:] == SENTINEL).all()), (name, t, "workspace written past the plan's size")
            res.append((out, [b.clone() for b in st.bufs]))
        (o0, b0), (o1, b1) = res
        assert torch.equal(o0.view(torch.int16), o1.view(torch.int16)), (name, t, fam, "NaN and stale runs differ")
        if t == bound:
            at_bound = (o0, b0)
        elif t > bound:  # clamped to the bound: the same output and the same stores as the call at the bound
            assert torch.equal(o0.view(torch.int16), at_bound[0].view(torch.int16)), (name, t)
            assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(b0, at_bound[1])), (name, t)


def _prefix(c, t):
    """case ``c`` cut to its first ``t`` stored tokens, with stored token ``t`` (its raw values) as the new one"""
    s = copy.copy(c)
    s.T = t
    s.kq, s.ks, s.vq, s.vs = c.kq[:, :, :t], c.ks[:t], c.vq[:, :, :t], c.vs[:t]
    s.kint, s.vint = c.kint[:, :, :t], c.vint[:, :, :t]
    if t < c.T:
        s.kn, s.vn = np.ascontiguousarray(c.kraw[:, :, t]), np.ascontiguousarray(c.vraw[:, :, t])
    return s


def test_graph_replay_across_a_ring_layout_change(K, tunable):
    """One captured step (decode_step_dev, the count + 1, the output copied into a per-step history row picked by the
    count) replayed across a 64-token tile edge where the ring's live tiles per wave and its live split count both change.
    Step n attends what the steps before it appended: every step within budget of the oracle, every appended slot the
    oracle's quantised token, and three steps bit-identical to an eager call at the same count on the same store."""
    name = "ring hd128 TG4, <16, true>"
    (B, Hq, Hkv, D), kinds, bound, knobs = ROUTES[name][:4]
    for key, val in knobs.items():
        tunable(key, val)
    p = route_plan(name)
    edge = next(t for t in A.dev_plan_changes(p) if p.live(t)[0] != p.live(t - 1)[0])  # the first change of tiles per wave
    t0, n = edge - 6, 12
    assert (edge - 1) % 64 == 0 and p.live(edge)[1] != p.live(edge - 1)[1], (edge, p.live(edge), p.live(edge - 1))
    c = A.make_case("probe", "decode", B, Hq, Hkv, t0 + n, 1, D, kinds, "f16", seed=29, probe_every=2,
                    splits=(p.live(t0)[0], p.live(t0 + n)[0]))
    cap = bound + 8
    st = Stores(K, _prefix(c, t0), cap, "nan")
    q = to_torch(np.ascontiguousarray(c.q[:, :, 0]), "f16")
    kn = torch.empty(B, Hkv, D, dtype=torch.float16, device="cuda")
    vn = torch.empty_like(kn)
    out = torch.empty_like(q)
    hist = torch.full((t0 + n + 1, B, Hq, D), float("nan"), dtype=torch.float16, device="cuda")
    ws = torch.full((K.decode_attn_workspace(B, Hq, Hkv, bound, D),), float("nan"), device="cuda")
    t_dev = torch.tensor([t0], dtype=torch.int32, device="cuda")
    plan = K.DecodeStepPlan(q, st.views[0], st.views[1], kinds[0], st.views[2], st.views[3], kinds[1], 1e-8)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture, on a scratch copy of the store
        sc = Stores(K, _prefix(c, t0), cap, "nan")
        ps = K.DecodeStepPlan(q, sc.views[0], sc.views[1], kinds[0], sc.views[2], sc.views[3], kinds[1], 1e-8)
        K.decode_step_dev(ps, q, kn, vn, t_dev, bound, out, ws, c.sm)
        hist.index_copy_(0, t_dev.long(), out.unsqueeze(0))
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    hist.fill_(float("nan"))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        K.decode_step_dev(plan, q, kn, vn, t_dev, bound, out, ws, c.sm)
        t_dev.add_(1)
        hist.index_copy_(0, t_dev.long(), out.unsqueeze(0))
    raw = lambda x, t: to_torch(np.ascontiguousarray(x[:, :, t]), "f16")
    for t in range(t0, t0 + n):
        kn.copy_(raw(c.kraw, t))
        vn.copy_(raw(c.vraw, t))
        graph.replay()
    torch.cuda.synchronize()
    assert int(t_dev.item()) == t0 + n
    for t in range(t0, t0 + n):
        s = _prefix(c, t)
        ref = s.reference()
        ok, r = A.check(got64(hist[t + 1]), ref, A.bound(s, ref, qplanes=True))
        assert ok, (t, p.live(t), r)
    for i, (qa, sc_) in enumerate(((c.kq, c.ks), (c.vq, c.vs))):  # every appended slot, bit for bit
        assert np.array_equal(to_numpy(st.views[2 * i][:, :, t0:t0 + n]), qa[:, :, t0:t0 + n]), i
        assert np.array_equal(to_numpy(st.views[2 * i + 1][t0:t0 + n]), sc_[t0:t0 + n]), i
        assert torch.equal(_bits(st.views[2 * i + 1][t0 + n:]), _bits(st.before[2 * i + 1][GUARD + t0 + n:GUARD + cap])), i
    t_eager = torch.zeros(1, dtype=torch.int32, device="cuda")
    for t in (t0, edge - 1, edge):
        kn.copy_(raw(c.kraw, t))
        vn.copy_(raw(c.vraw, t))
        t_eager.fill_(t)
        oe = torch.full_like(q, float("nan"))
        K.decode_step_dev(plan, q, kn, vn, t_eager, bound, oe, ws, c.sm)
        torch.cuda.synchronize()
        assert torch.equal(oe.view(torch.int16), hist[t + 1].view(torch.int16)), t
