"""Pins oracle.decode_attention (scope row N1, second form) on the CPU: the reference has no
attention code of its own — `to_past_key_values` (ops.py:345-355) hands dequantised tensors to
the HF model — so the oracle is checked against torch's scaled_dot_product_attention (what HF
runs) over the oracle's own dequantised values plus the exact new token."""
import numpy as np
import pytest
import torch

from oracle import kvq_oracle as O


@pytest.mark.parametrize("B,Hq,Hkv,T,D", [(1, 4, 4, 37, 64), (2, 8, 2, 130, 32), (1, 6, 3, 1, 16), (1, 2, 2, 0, 8)])
@pytest.mark.parametrize("kinds", [("int8", "int4"), ("int4", "int8")])
@pytest.mark.parametrize("with_new", [True, False])
def test_decode_attention_oracle_vs_torch_sdpa(B, Hq, Hkv, T, D, kinds, with_new):
    if T == 0 and not with_new:
        pytest.skip("nothing to attend to")
    rng = np.random.default_rng(B * 1000 + T)
    k = rng.standard_normal((1, B, Hkv, T, D)).astype(np.float16)
    v = rng.standard_normal((1, B, Hkv, T, D)).astype(np.float16)
    kq, _, ks = O.quantize_tokens(k, kinds[0])
    vq, _, vs = O.quantize_tokens(v, kinds[1])
    q = rng.standard_normal((B, Hq, D)).astype(np.float16)
    kn = rng.standard_normal((B, Hkv, D)).astype(np.float16) if with_new else None
    vn = rng.standard_normal((B, Hkv, D)).astype(np.float16) if with_new else None
    sm = 1.0 / np.sqrt(D)
    got = O.decode_attention(q, kq[0], ks[0], kinds[0], vq[0], vs[0], kinds[1], D, sm, kn, vn)

    kd = torch.from_numpy(O.dequantize_tokens(kq, ks, kinds[0], D, "f16")[0]).double()
    vd = torch.from_numpy(O.dequantize_tokens(vq, vs, kinds[1], D, "f16")[0]).double()
    if with_new:
        kd = torch.cat([kd, torch.from_numpy(kn).double()[:, :, None]], dim=2)
        vd = torch.cat([vd, torch.from_numpy(vn).double()[:, :, None]], dim=2)
    rep = Hq // Hkv
    ref = torch.nn.functional.scaled_dot_product_attention(
        torch.from_numpy(q).double()[:, :, None], kd.repeat_interleave(rep, dim=1), vd.repeat_interleave(rep, dim=1),
        scale=sm)[:, :, 0].numpy()
    assert np.allclose(got, ref, rtol=1e-9, atol=1e-11)


def _sdpa_extend(q, kq, ks, vq, vs, kinds, D, sm, kn, vn):
    """float64 torch SDPA over the oracle's dequantised store + the chunk, with HF's lower-right causal mask written out
    as a boolean mask: key j (store first, then chunk) is visible to query row s iff j < T + s + 1."""
    T, S = ks.shape[-1], q.shape[2]
    kd = torch.from_numpy(O.dequantize_tokens(kq, ks, kinds[0], D, "f16")[0]).double() if T else torch.zeros(*kn.shape[:2], 0, D).double()
    vd = torch.from_numpy(O.dequantize_tokens(vq, vs, kinds[1], D, "f16")[0]).double() if T else torch.zeros(*vn.shape[:2], 0, D).double()
    kd = torch.cat([kd, torch.from_numpy(kn).double()], dim=2)
    vd = torch.cat([vd, torch.from_numpy(vn).double()], dim=2)
    rep = q.shape[1] // kn.shape[1]
    mask = torch.arange(T + S)[None, :] < (T + torch.arange(S)[:, None] + 1)
    qt = torch.from_numpy(q).double()
    ref = torch.nn.functional.scaled_dot_product_attention(
        qt, kd.repeat_interleave(rep, dim=1), vd.repeat_interleave(rep, dim=1), attn_mask=mask, scale=sm)
    upper_left = torch.nn.functional.scaled_dot_product_attention(
        qt, kd.repeat_interleave(rep, dim=1), vd.repeat_interleave(rep, dim=1), is_causal=True, scale=sm)
    return ref.numpy(), upper_left.numpy()


@pytest.mark.parametrize("B,Hkv,nq,T,S,D", [(1, 2, 1, 0, 5, 16), (2, 2, 3, 37, 1, 32), (1, 1, 7, 70, 6, 16),
                                             (2, 3, 3, 1, 9, 8), (1, 2, 7, 0, 1, 16), (1, 2, 1, 130, 4, 64)])
@pytest.mark.parametrize("kinds", [("int8", "int4"), ("int4", "int8")])
def test_extend_attention_oracle_vs_torch_sdpa(B, Hkv, nq, T, S, D, kinds):
    """Pins oracle.extend_attention (the float64 reference of kvq_extend_attn) on the CPU: torch SDPA in float64 with an
    explicit lower-right causal mask over the same dequantised values. S = 1 is a decode step with the new token given:
    equal to oracle.decode_attention. With a past and more than one chunk token, torch's `is_causal=True` (upper-left
    aligned: row s sees keys j <= s) is a different function, so the oracle cannot follow that convention by mistake."""
    Hq = Hkv * nq
    rng = np.random.default_rng(B * 1000 + T * 10 + S + nq)
    k = rng.standard_normal((1, B, Hkv, T, D)).astype(np.float16)
    v = rng.standard_normal((1, B, Hkv, T, D)).astype(np.float16)
    if T:
        kq, _, ks = O.quantize_tokens(k, kinds[0])
        vq, _, vs = O.quantize_tokens(v, kinds[1])
    else:
        kq = np.zeros((1, B, Hkv, 0, D if kinds[0] == "int8" else D // 2), np.int8 if kinds[0] == "int8" else np.uint8)
        vq = np.zeros((1, B, Hkv, 0, D if kinds[1] == "int8" else D // 2), np.int8 if kinds[1] == "int8" else np.uint8)
        ks = vs = np.zeros((1, 0), np.float32)
    q = (rng.standard_normal((B, Hq, S, D)) * 2.0).astype(np.float16).astype(np.float32)
    kn = rng.standard_normal((B, Hkv, S, D)).astype(np.float16).astype(np.float32)
    vn = rng.standard_normal((B, Hkv, S, D)).astype(np.float16).astype(np.float32)
    sm = 1.0 / np.sqrt(D)
    got = O.extend_attention(q, kq[0], ks[0], kinds[0], vq[0], vs[0], kinds[1], D, sm, kn, vn)
    ref, upper_left = _sdpa_extend(q, kq, ks, vq, vs, kinds, D, sm, kn, vn)
    assert np.allclose(got, ref, rtol=1e-9, atol=1e-11)
    if S == 1:
        dec = O.decode_attention(q[:, :, 0], kq[0], ks[0], kinds[0], vq[0], vs[0], kinds[1], D, sm, kn[:, :, 0], vn[:, :, 0])
        assert np.array_equal(got[:, :, 0], dec)
    if T > 0 and S > 1:
        assert not np.allclose(got, upper_left, rtol=1e-3, atol=1e-3)
    if T == 0:  # no past: lower-right and upper-left alignment coincide
        assert np.allclose(got, upper_left, rtol=1e-9, atol=1e-11)


@pytest.mark.parametrize("mode,T,S,W", [("decode", 70, 1, 1), ("decode", 70, 1, 5), ("decode", 70, 1, 71), ("decode", 0, 1, 3),
                                        ("nonew", 70, 1, 1), ("nonew", 70, 1, 9), ("extend", 37, 12, 5), ("extend", 0, 20, 7),
                                        ("extend", 130, 4, 1), ("extend", 9, 30, 40), ("extend", 50, 8, 58)])
def test_windowed_oracle_vs_window_ref_and_brute_force(mode, T, S, W):
    """oracle.decode_attention / extend_attention with ``window`` against tests/attn_ref.attention (the
    float64 model the attention GPU tests use) and against a softmax written out key by key with HF's band (query at
    position p sees key k iff p - W < k <= p; decode p = T with the new token, T - 1 without; extend p = T + s). A window
    that cuts nothing gives the unwindowed oracle's bits."""
    from tests.attn_ref import attention, dequant
    B, Hq, Hkv, D, kinds = 1, 4, 2, 16, ("int8", "int4")
    rng = np.random.default_rng(T * 100 + S * 10 + W)
    k = rng.standard_normal((1, B, Hkv, T, D)).astype(np.float16)
    v = rng.standard_normal((1, B, Hkv, T, D)).astype(np.float16)
    kq, _, ks = O.quantize_tokens(k, kinds[0])
    vq, _, vs = O.quantize_tokens(v, kinds[1])
    kq, ks, vq, vs = kq[0], ks[0], vq[0], vs[0]
    Sn = 0 if mode == "nonew" else S
    q = (rng.standard_normal((B, Hq, S, D)) * 2.0).astype(np.float16).astype(np.float64)
    kn = rng.standard_normal((B, Hkv, Sn, D)).astype(np.float16).astype(np.float64)
    vn = rng.standard_normal((B, Hkv, Sn, D)).astype(np.float16).astype(np.float64)
    sm = 1.0 / np.sqrt(D)
    kd = np.concatenate([dequant(kq, ks, kinds[0], D), kn], axis=2)
    vd = np.concatenate([dequant(vq, vs, kinds[1], D), vn], axis=2)
    if mode == "extend":
        got = O.extend_attention(q, kq, ks, kinds[0], vq, vs, kinds[1], D, sm, kn, vn, window=W)
        full = O.extend_attention(q, kq, ks, kinds[0], vq, vs, kinds[1], D, sm, kn, vn)
        pos = T + np.arange(S)
    else:
        a = (kn[:, :, 0], vn[:, :, 0]) if Sn else (None, None)
        got = O.decode_attention(q[:, :, 0], kq, ks, kinds[0], vq, vs, kinds[1], D, sm, *a, window=W)[:, :, None]
        full = O.decode_attention(q[:, :, 0], kq, ks, kinds[0], vq, vs, kinds[1], D, sm, *a)[:, :, None]
        pos = np.array([T if Sn else T - 1])
    assert np.allclose(got, attention(q, kd, vd, pos, sm, W), rtol=1e-12, atol=1e-14)
    brute = np.empty_like(got)
    for b in range(B):
        for h in range(Hq):
            for r, p in enumerate(pos):
                keys = [kk for kk in range(kd.shape[2]) if p - W < kk <= p]
                sc = np.array([q[b, h, r] @ kd[b, h // (Hq // Hkv), kk] * sm for kk in keys])
                e = np.exp(sc - sc.max())
                brute[b, h, r] = sum(e[i] * vd[b, h // (Hq // Hkv), kk] for i, kk in enumerate(keys)) / e.sum()
    assert np.allclose(got, brute, rtol=1e-12, atol=1e-14)
    if W > pos[-1]:  # the band reaches key 0 for every row: the unwindowed oracle's bits
        assert np.array_equal(got, full)
    else:
        assert not np.allclose(got, full, rtol=1e-6, atol=1e-8)
