"""tests/attn_ref.py, the float64 attention every attention test compares against, is itself checked (CPU): without starts and
modifiers it equals the project's oracle (``oracle.kvq_oracle.decode_attention`` / ``extend_attention``) bit for bit, and with
per-row starts, a soft cap and sinks it agrees to 1e-12 with a brute-force masked softmax written here (a dense [S, N] mask
from the visibility rule, plain ``np.exp``, one row at a time)."""
import numpy as np
import pytest

from oracle import kvq_oracle as O
from tests import attn_cases as A
from tests import attn_ref as R

B, HQ, HKV, T, D = 2, 8, 2, 70, 64
KINDS = ("int8", "int4")
SM = D ** -0.5
CAP = 5.0


def _case(mode, dtype, S, W, starts, with_new, seed):
    rng = np.random.default_rng(seed)
    rand = lambda *shape: A.narrow(rng.standard_normal(shape), dtype)
    if mode == "extend":
        kn, vn = rand(B, HKV, S, D), rand(B, HKV, S, D)
    else:
        kn, vn = (rand(B, HKV, D), rand(B, HKV, D)) if with_new else (None, None)
    return A.Case(mode, dtype, KINDS, SM, rand(B, HQ, S if mode == "extend" else 1, D), rand(B, HKV, T, D), rand(B, HKV, T, D),
                  kn, vn, {}, window=W, kv_start=starts)


def _cases(dtype, S, W, starts):
    seed = S * 100 + W + (0 if starts is None else starts[1])
    return [_case("decode", dtype, 1, W, starts, True, seed), _case("decode", dtype, 1, W, starts, False, seed + 1),
            _case("extend", dtype, S, W, starts, True, seed + 2)]


def _brute(c, softcap, sinks):
    """masked softmax of case ``c``, row by row: [B,Hq,S,D]"""
    kd, vd = R.keys_values(c)
    q = A.widen(c.q, c.dtype)
    N = kd.shape[2]
    pos = [c.T + s for s in range(c.S)] if c.mode == "extend" else [N - 1]
    mask = np.zeros((c.B, c.S, N), bool)
    for b in range(c.B):
        for s, p in enumerate(pos):
            for k in range(N):
                mask[b, s, k] = max(c.kv_start[b] if c.kv_start else 0, p - c.window + 1 if c.window else 0) <= k <= p
    out = np.zeros((c.B, c.Hq, c.S, c.D))
    for b in range(c.B):
        for h in range(c.Hq):
            g = h // (c.Hq // c.Hkv)
            for s in range(c.S):
                keys = np.nonzero(mask[b, s])[0]
                if not len(keys):
                    continue  # a row that sees no key: zeros
                x = kd[b, g, keys] @ q[b, h, s] * c.sm
                if softcap:
                    x = softcap * np.tanh(x / softcap)
                m = x.max() if sinks is None else max(x.max(), float(sinks[h]))
                w = np.exp(x - m)
                den = w.sum() + (0.0 if sinks is None else np.exp(float(sinks[h]) - m))
                out[b, h, s] = (w / den) @ vd[b, g, keys]
    return out, mask


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("W", [0, 7, 40])
@pytest.mark.parametrize("S", [1, 5])
def test_equals_the_oracle_bit_for_bit(S, W, dtype):
    for c in _cases(dtype, S, W, None):
        w = lambda x: None if x is None else A.widen(x, dtype)
        args = (c.kq, c.ks, KINDS[0], c.vq, c.vs, KINDS[1], D, SM, w(c.kn), w(c.vn))
        kd, vd = R.dequant(c.kq, c.ks, KINDS[0], D, dtype), R.dequant(c.vq, c.vs, KINDS[1], D, dtype)
        if c.mode == "decode":
            want = O.decode_attention(w(c.q[:, :, 0]), *args, kv_dtype=dtype, window=W)
            got = R.decode(kd, vd, w(c.q[:, :, 0]), w(c.kn), w(c.vn), T, W, SM)
        else:
            want = O.extend_attention(w(c.q), *args, kv_dtype=dtype, window=W)
            got = R.extend(kd, vd, w(c.q), w(c.kn), w(c.vn), T, W, SM)
        assert want.dtype == np.float64 and np.array_equal(got, want), (c.mode, c.kn is None)
        assert np.array_equal(R.of_case(c), want) and np.array_equal(c.reference(), want), (c.mode, c.kn is None)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("starts", [None, [0, 33], [0, 70]], ids=["no starts", "starts 0,33", "starts 0,70"])
@pytest.mark.parametrize("W", [0, 7, 40])
@pytest.mark.parametrize("S", [1, 5])
def test_equals_a_brute_force_masked_softmax(S, W, starts, dtype):
    """starts, cap and sinks, alone and together; a row that sees no key is exactly zero, also with a sink"""
    rng = np.random.default_rng(S + W)
    sinks = (2.0 * rng.standard_normal(HQ)).astype(np.float32)
    sinks[2], sinks[5] = -1e30, 9.0  # no effect; above every score
    dead_rows = 0
    for c in _cases(dtype, S, W, starts):
        for softcap, sk in ((0.0, None), (CAP, None), (0.0, sinks), (CAP, sinks)):
            want, mask = _brute(c, softcap, sk)
            got = R.of_case(c, softcap, sk)
            got = got[:, :, None] if c.mode == "decode" else got
            assert np.abs(got - want).max() <= 1e-12, (c.mode, c.kn is None, softcap, sk is not None)
            dead = ~mask.any(axis=-1)  # [B,S]
            assert (got.transpose(0, 2, 1, 3)[dead] == 0).all() and np.array_equal(R.visible(c), mask)
            dead_rows += int(dead.sum())
        if starts is not None:  # the wrappers on arrays clamp the starts as the case does
            kd, vd = R.dequant(c.kq, c.ks, KINDS[0], D, dtype), R.dequant(c.vq, c.vs, KINDS[1], D, dtype)
            w = lambda x: None if x is None else A.widen(x, dtype)
            fn, q = (R.decode, w(c.q[:, :, 0])) if c.mode == "decode" else (R.extend, w(c.q))
            assert np.array_equal(fn(kd, vd, q, w(c.kn), w(c.vn), T, W, SM, starts, CAP, sinks), R.of_case(c, CAP, sinks))
    assert (dead_rows > 0) == (starts == [0, 70])  # decode without the new token at position 69 under a start of 70
