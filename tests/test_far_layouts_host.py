"""CPU checks of tests/far_layouts.py: every layout of the table is far, aligned and safe (see that module's docstring),
every addressing model of the discrimination test moves a block on some layout, and the guard-boundary strides sit on the
two sides of the library's own bounds (restated here from csrc/kvq_quant.hip, csrc/kvq_evict.hip and csrc/attn/host.inc).
No GPU, no torch."""
import pytest

from tests import far_layouts as F

LAYOUTS = list(F.TABLE.values())
IDS = [l.name for l in LAYOUTS]


@pytest.mark.parametrize("layout", LAYOUTS, ids=IDS)
def test_layout_is_far_aligned_and_safe(layout):
    assert layout.arena == F.ARENA_BYTES
    for t in layout.t.values():
        assert not F.alignment_faults(t), F.alignment_faults(t)
        for start in t.blocks().values():
            assert 0 <= start and start + t.block_bytes <= layout.arena, (t, start)
        if t.far:
            rep = F.far_report(t)
            assert all(rep.values()), (layout.name, t, rep)
    assert not F.safety_faults(layout), F.safety_faults(layout)[:5]


def test_bases_leave_room_for_stacked_negative_wraps():
    """two negative int32 wraps of byte products (each down to -2^31) stay inside; so does one of an fp32 ELEMENT offset
    (down to -2^33 bytes)"""
    assert F.P1 >= (1 << 32) + 64 * F.MiB and F.P4 >= (1 << 33) + 64 * F.MiB
    for layout in LAYOUTS:
        for t in layout.t.values():
            if t.far:
                assert t.base >= (F.P4 if t.esz == 4 else F.P1), (layout.name, t)


def test_fill_pattern_is_a_decoy_in_every_dtype():
    import numpy as np
    word = np.full(4, F.FILL, np.uint8)
    assert word.view(np.int8)[0] == 90 and (F.FILL >> 4, F.FILL & 15) == (5, 10)
    assert float(word.view(np.float16)[0]) == 203.25
    assert 1e16 < float(word.view(np.float32)[0]) < 2e16
    assert int(word.view(np.int32)[0]) > 1 << 30  # no token index of any test reaches it


@pytest.mark.parametrize("model", [m for m in F.MODELS if m != "exact"])
def test_every_wrong_model_moves_a_block_somewhere(model):
    """...and on every far tensor at least one of the models does: no far tensor is blind to all of them"""
    hit = [l.name for l in LAYOUTS if any(F.moved(t, model) for t in l.t.values())]
    assert hit, model
    for layout in LAYOUTS:
        for t in layout.t.values():
            if t.far:
                assert any(F.moved(t, m) for m in F.MODELS if m != "exact"), (layout.name, t)


def test_wrong_starts_cover_the_models():
    """the safety check's candidate set contains every address the discrimination test's models produce"""
    for layout in LAYOUTS:
        for t in layout.t.values():
            wrong = F.wrong_starts(t)
            for m in F.MODELS:
                for idx in F.moved(t, m):
                    assert F.block_start(t, idx, m) in wrong, (layout.name, t, m, idx)


def test_packed_views_overlap_nothing():
    """every logical row of every tensor of a layout is its own bytes: the arena sweep can restore them one by one"""
    for layout in LAYOUTS:
        spans = sorted((a, a + t.row_bytes) for t in layout.t.values() for _, a in t.rows())
        assert all(b0 >= a1 for (_, a1), (b0, _) in zip(spans, spans[1:])), layout.name


# ---------------------------------------------------------------------------------------------------- guard boundaries
LIMIT = 1 << 31


def test_under_and_at_are_adjacent_multiples():
    for count, fixed, align in ((7, 1024, 16), (135, 2048, 16), (32, 0, 16), (600, 0, 16), (600, 0, 8)):
        under, at = F.under_and_at(LIMIT, count, fixed, align)
        assert under % align == 0 and at % align == 0 and at - under == align
        assert count * under + fixed < LIMIT <= count * at + fixed


@pytest.mark.parametrize("kind", ["int8", "int4"])
def test_tile_guard_strides(kind):
    """quant_route: span_in = (R - 1) * is.h * 2 + tt * D * 2, span_q = (R - 1) * qs.h + tt * Dq, Tile iff both < 2^31"""
    G, B, H, T, D = F.TILE_SHAPE
    R, tt, Dq = B * H, 4, F.packed(kind, D)
    assert (D, R) == (128, 8)
    g = F.tile_guard(kind)
    for side, want in ((0, True), (1, False)):
        assert ((R - 1) * g["in"][side] + tt * D * 2 < LIMIT) is want
        assert ((R - 1) * g["q"][side] + tt * Dq < LIMIT) is want
        assert g["in"][side] % 16 == 0 and g["q"][side] % 16 == 0


def test_split_guard_strides():
    """split_walk_ok: (R - 1) * is.h * 2 + 8 * D * 2 and (R - 1) * qs.h + 8 * D, both < 2^31; R * D > 16,384 (not a tile)"""
    G, B, H, T, D = F.SPLIT_SHAPE
    R = B * H
    assert D == 128 and R * D > 16384 and (R + 7) // 8 < 65536
    g = F.split_guard()
    for side, want in ((0, True), (1, False)):
        assert ((R - 1) * g["in"][side] + 8 * D * 2 < LIMIT) is want
        assert ((R - 1) * g["q"][side] + 8 * D < LIMIT) is want


def test_pool_guard_strides():
    """pool_route: Wave iff chunk_size * isb.t < 2^31 (chunk 32 at D = 128: 4 lane groups of 8 rows)"""
    g = F.POOL_GUARD
    assert g["D"] == 128 and g["chunk"] % 4 == 0 and g["chunk"] // 4 in (8, 16)
    under, at = F.pool_guard()
    assert g["chunk"] * under < LIMIT <= g["chunk"] * at and under % 16 == 0 and at % 16 == 0


def test_row_guard_strides():
    """decode_attn_impl: T * st.t < 2^31 for K and for V"""
    under, at = F.row_guard()
    assert F.ROW_GUARD_T * under < LIMIT <= F.ROW_GUARD_T * at and under % 16 == 0 and at % 16 == 0
    for side, st in (("under", under), ("at", at)):
        lay = F.TABLE[f"guard rows {side}"]
        assert lay["k_store"].strides[2] == st and lay["v_store"].strides[2] == st
