"""CPU proof that the eviction edge families (tests/evict_cases.py) can catch the mistakes a mean-pool kernel can make.

test_gpu_evict_edges.py compares every eviction route with the oracle bit for bit on these families. That means
something only if the families tell a wrong kernel from a right one, and for the 16-bit mean-pool the suite's seeded
random data does not: the fp32 sums of another row order differ in about 1 % of outputs and the final rounding to 16
bits hides next to all of them: 1 of 16,384 stored outputs changes (test_seeded_heavy_data_is_blind_to_the_row_order
keeps that finding). Here numpy restatements of the mistakes (`evict_cases.pooled`) stand in for the kernel.

Share of the pooled stored outputs of the whole chunks that each order mutant changes, on EVERY `order` case the GPU
tests run (`evict_cases.ORDER_CASES`, from which test_gpu_evict_edges.py builds its data: B 1, H 2, three whole chunks).
`groups` = the lane groups of the shape's chunk_pool_wave_k instantiation, where it has one; `lowp` = a 16-bit
accumulator. The condition is >= 0.5 for each. The lowest measured are the chunks of 7 rows, where a big value meets few
rows: 0.550 (bf16, D 5, swapped), 0.556 (bf16, D 64, swapped), 0.567 (bf16, D 5, pairwise); every chunk of 16 rows or
more is at 0.681 or above. `pytest -s` prints the table.

    dtype  G  D    chunk  reversed swapped  pairwise exact    groups   lowp
    f16    2  128  64     0.958    0.962    0.980    0.983    0.911    0.998
    f16    2  128  32     0.965    0.952    0.955    0.975    0.868    0.990
    f16    2  64   64     0.962    0.943    0.969    0.974    0.928    0.996
    f16    2  64   128    0.948    0.941    0.986    0.983    0.964    1.000
    f16    2  256  32     0.968    0.948    0.961    0.983    0.745    0.995
    f16    2  256  16     0.978    0.927    0.917    0.982    0.733    0.983
    f16    2  64   7      0.947    0.594    0.712    0.935    -        0.879
    f16    2  64   24     0.971    0.952    0.932    0.980    -        0.993
    f16    2  64   40     0.966    0.957    0.948    0.983    -        0.996
    bf16   2  128  64     0.880    0.747    0.937    0.940    0.865    0.995
    bf16   2  128  32     0.891    0.780    0.922    0.931    0.861    0.983
    bf16   2  64   64     0.889    0.733    0.927    0.938    0.880    0.993
    bf16   2  64   128    0.849    0.721    0.952    0.935    0.882    0.995
    bf16   2  256  32     0.914    0.782    0.919    0.940    0.697    0.983
    bf16   2  256  16     0.923    0.788    0.859    0.935    0.681    0.963
    bf16   2  64   7      0.908    0.556    0.664    0.910    -        0.828
    bf16   2  64   24     0.914    0.793    0.854    0.939    -        0.982
    bf16   2  64   40     0.908    0.781    0.906    0.932    -        0.990
    f32    2  64   7      0.956    0.622    0.767    0.969    -        -
    f32    2  64   24     0.995    0.973    0.958    1.000    -        -
    f32    2  64   40     1.000    0.983    0.973    1.000    -        -
    f32    2  128  64     1.000    0.992    0.994    0.999    -        -
    f16    2  5    7      0.933    0.600    0.683    0.917    -        0.900
    f16    2  128  24     0.972    0.947    0.938    0.979    -        0.987
    bf16   2  5    7      0.917    0.550    0.567    0.900    -        0.783
    bf16   2  128  24     0.919    0.790    0.887    0.941    -        0.984
    f32    2  5    7      0.950    0.650    0.750    0.950    -        -
    f32    2  128  24     0.997    0.975    0.962    0.999    -        -
    f16    4  128  64     0.964    0.953    0.979    0.980    0.904    0.996
    bf16   4  128  64     0.891    0.766    0.926    0.932    0.858    0.992

Reciprocal multiply on the f32 `division` cases (condition >= 0.1): chunk 7 0.528, chunk 24 0.332, chunk 40 0.203.
The other families need one changed output from their matching mutant: `ragged_tail` from a ragged chunk that reads on
into the kept rows (it changes every column) and from a divisor of n; `denormal_mean` from ties rounded away from zero,
subnormal results flushed to zero (f16) and an accumulator that starts at -0.0.
"""
import numpy as np
import pytest

from oracle import kvq_oracle as O
from tests import evict_cases as C
from tests.util import seeded_kv

ORDER_MUTANTS = ("reversed", "swapped", "pairwise", "exact", "groups", "lowp")
N_FULL = 3  # whole chunks of every case; the pooled rows behind them belong to the ragged chunk


def _case_id(case):
    return f"{case['dtype']}-G{case.get('G', 2)}-D{case['D']}-c{case['chunk']}"


def _oracle_pooled(x, dtype, chunk, keep):
    old = x.shape[-2] - min(keep, x.shape[-2])
    with np.errstate(over="ignore"):  # denormal_mean overflows an fp32 sum on purpose
        return O.chunk_summarize_kv(x, chunk, keep, dtype=C.odt(dtype))[..., :(old + chunk - 1) // chunk, :]


def order_shares(case):
    """mutant -> share of the whole chunks' pooled outputs it changes. `groups` only where the shape has a wave
    instantiation (its lane groups), `lowp` only for the 16-bit types (for f32 it is the oracle's sum)."""
    dtype, chunk, D = case["dtype"], case["chunk"], case["D"]
    x = C.order(**case)
    ref = C.pooled(x, dtype, chunk, 4)
    assert np.isfinite(C.widen(ref, dtype)).all()
    mutants = [m for m in ORDER_MUTANTS if (m != "groups" or (dtype != "f32" and (D, chunk) in C.WAVE_SHAPES)) and (m != "lowp" or dtype != "f32")]
    return {m: C.changed_share(ref[..., :N_FULL, :], C.pooled(x, dtype, chunk, 4, how=m, groups=C.WAVE_GROUPS.get(D))[..., :N_FULL, :])
            for m in mutants}


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_default_restatement_is_the_oracle(dtype):
    """`pooled` with its defaults is the oracle's sum on every family, so that a mutant differs by its mistake alone"""
    cases = [(C.order(dtype, 16, ragged=5), 16), (C.ragged_tail(dtype, 7, 1), 7), (C.ragged_tail(dtype, 16, 9), 16),
             (C.denormal_mean(dtype, 64), 64), (C.denormal_mean(dtype, 24, ragged=3), 24), (C.bits_case(dtype)[0], 64)]
    if dtype == "f32":
        cases.append((C.division(7), 7))
    for x, chunk in cases:
        keep = 256 if x.shape[-2] == 320 else 4
        got, ref = C.pooled(x, dtype, chunk, keep), _oracle_pooled(x, dtype, chunk, keep)
        assert C.changed_share(got, ref) == 0.0
        assert not np.isnan(C.widen(ref, dtype)).any()  # pooled outputs of the families are never NaN


@pytest.mark.parametrize("case", C.ORDER_CASES, ids=[_case_id(c) for c in C.ORDER_CASES])
def test_order_rejects_every_order_mutant(case):
    """every `order` case the GPU tests run (evict_cases.ORDER_CASES; they build their data from the same entries)"""
    shares = order_shares(case)
    print(f"    {case['dtype']:<6} {case.get('G', 2):<2} {case['D']:<4} {case['chunk']:<6} "
          + " ".join(f"{shares[m]:<8.3f}" if m in shares else f"{'-':<8}" for m in ORDER_MUTANTS))
    assert min(shares.values()) >= 0.5, shares


def test_seeded_heavy_data_is_blind_to_the_row_order():
    """The finding behind this file: on the suite's own f16 data a reversed sum changes some fp32 sums and (next to)
    none of the stored outputs, so a kernel with the wrong row order passes every seeded_kv test."""
    x = seeded_kv((2, 1, 8, 512, 128), "f16", 31, "heavy")
    ref, rev = C.pooled(x, "f16", 64, 0), C.pooled(x, "f16", 64, 0, how="reversed")
    assert C.changed_share(ref, rev) < 0.001  # measured: 1 of 16,384
    y = C.order("f16", 64, D=128)
    assert C.changed_share(C.pooled(y, "f16", 64, 4), C.pooled(y, "f16", 64, 4, how="reversed")) >= 0.5


@pytest.mark.parametrize("chunk", [7, 24, 40])
def test_division_rejects_the_reciprocal_and_the_row_count(chunk):
    x = C.division(chunk)
    ref = C.pooled(x, "f32", chunk, 4)
    share = C.changed_share(ref, C.pooled(x, "f32", chunk, 4, div="recip"))
    print(f"chunk {chunk}: reciprocal multiply changes {share:.3f}")
    assert share >= 0.1
    by_n = C.pooled(x, "f32", chunk, 4, div="n")
    assert C.changed_share(ref[..., :-1, :], by_n[..., :-1, :]) == 0.0
    assert C.changed_share(ref[..., -1, :], by_n[..., -1, :]) >= 0.9  # the ragged chunk alone, and all of it


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("chunk,ragged", [(64, 1), (64, 9), (16, 9), (7, 1), (24, 17)])
def test_ragged_tail_rejects_reading_past_the_old_region(dtype, chunk, ragged):
    x = C.ragged_tail(dtype, chunk, ragged)
    ref, over = C.pooled(x, dtype, chunk, 4), C.pooled(x, dtype, chunk, 4, ragged="overread")
    assert np.isfinite(C.widen(ref, dtype)).all()
    assert C.changed_share(ref[..., :-1, :], over[..., :-1, :]) == 0.0
    assert C.changed_share(ref[..., -1, :], over[..., -1, :]) == 1.0  # every column sees 65504, NaN or inf
    assert C.changed_share(ref[..., -1, :], C.pooled(x, dtype, chunk, 4, div="n")[..., -1, :]) >= 0.9


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("chunk", [64, 16, 24])
def test_denormal_mean_rejects_rounding_and_zero_mistakes(dtype, chunk):
    x = C.denormal_mean(dtype, chunk)
    ref = C.pooled(x, dtype, chunk, 4)
    w = C.widen(ref, dtype)
    D = x.shape[-1]
    assert not np.isnan(w).any()
    zero = np.ascontiguousarray(ref[..., 1, :D // 2]).view(np.uint8)
    assert not zero.any()  # a chunk of -0.0 only pools to +0.0 ...
    assert C.changed_share(ref, C.pooled(x, dtype, chunk, 4, how="negzero")) > 0  # ... and an accumulator of -0.0 does not
    d = np.arange(D)
    assert np.isposinf(w[..., 2, d % 3 != 2]).all()  # +inf in a row, and the fp32 sum that overflows
    if dtype == "f32":
        return
    if chunk in (64, 16):
        assert C.count_ties(x, dtype, chunk, 4) >= 16
        assert C.changed_share(ref, C.pooled(x, dtype, chunk, 4, rounding="away")) > 0
    if dtype == "f16":
        sub = (np.ascontiguousarray(ref).view(np.uint16) & 0x7C00) == 0
        assert (sub & (w != 0)).sum() >= 64  # subnormal results
        assert C.changed_share(ref, C.pooled(x, dtype, chunk, 4, rounding="ftz")) > 0


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_bits_holds_every_pattern(dtype):
    x, chunk, keep = C.bits_case(dtype)
    assert x.shape == (1, 1, 2, 320, 128)
    tail = np.ascontiguousarray(x[..., chunk:, :])
    if dtype != "f32":
        assert np.array_equal(np.sort(tail.view(np.uint16).ravel()), np.arange(1 << 16, dtype=np.uint16))
    else:
        u = tail.view(np.uint32).ravel()
        nan = ((u & 0x7F800000) == 0x7F800000) & ((u & 0x007FFFFF) != 0)
        assert (nan & ((u & 0x00400000) == 0)).sum() > 1000 and (nan & ((u & 0x00400000) != 0)).sum() > 1000
        assert (((u & 0x7F800000) == 0) & ((u & 0x007FFFFF) != 0)).sum() > 1000
        for word in (0x0, 0x80000000, 0x7F800000, 0xFF800000, 0x1, 0x007FFFFF, 0x7F800001):
            assert (u == word).any()
    # the oracle hands the tail through as it is
    out = O.chunk_summarize_kv(x, chunk, keep, dtype=C.odt(dtype))
    assert np.array_equal(np.ascontiguousarray(out[..., 1:, :]).view(np.uint8), tail.view(np.uint8))
