"""The two checks tests/test_gpu_far_offsets.py makes after every call — the logical values against the oracle, and the
sweep of the arena for anything but 0x5A outside the restored regions — run on the CPU against a small addressing emulator,
to show that they reject 32-bit addressing on every far layout where it moves an address. No GPU.

The arena is sparse (a dict of 64 KiB pages over the 17.5 GiB address range). The emulator performs the three shapes of
access the kernels make, block by block (a block: what lies behind one far index tuple), with the addressing model as a
parameter (tests/far_layouts.MODELS):

    read     out[idx] = arena[block(idx)]: a kernel's loads             (gathers, dequantise and attention inputs)
    write    arena[block(idx)] = data[idx]: a kernel's stores           (codes, dequantised rows, pooled rows)
    update   arena[block(idx)] += 1 in place: read-modify-write         (scale tables, accumulated mass)
    stray    write with exact addresses, PLUS a second store at the model's address (a stale prefetch, a duplicated tail)

Model by model, on every (layout, tensor) where the model moves at least one block — tests/test_far_layouts_host.py
guarantees such a layout for each —, the check that rejected it:

    model         read     write            update           stray
    exact         passes   passes           passes           passes
    sum_i32       values   values + sweep   values + sweep   sweep
    sum_u32       values   values + sweep   values + sweep   sweep
    product_i32   values   values + sweep   values + sweep   sweep
    product_u32   values   values + sweep   values + sweep   sweep
    stride_i32    values   values + sweep   values + sweep   sweep
    stride_u32    values   values + sweep   values + sweep   sweep
    elem_i32      values   values + sweep   values + sweep   sweep
    elem_u32      values   values + sweep   values + sweep   sweep

(`values`: the wrong block held 0x5A, or the right one still does; `sweep`: the wrong block is dirty after the true regions
were restored. A stray store leaves every value right: only the sweep sees it.) No model ever leaves the arena: that is the
layouts' safety property, asserted here as well."""
import numpy as np
import pytest

from tests import far_layouts as F

PAGE = 1 << 16


class SparseArena:
    """``size`` bytes of FILL; pages are materialised when written"""

    def __init__(self, size):
        self.size, self.pages = size, {}

    def _spans(self, addr, n):
        assert 0 <= addr and addr + n <= self.size, ("outside the arena: a fault on the GPU", addr, n)
        while n:
            page, off = divmod(addr, PAGE)
            m = min(n, PAGE - off)
            yield page, off, m
            addr, n = addr + m, n - m

    def read(self, addr, n):
        out = [self.pages[p][o:o + m] if p in self.pages else np.full(m, F.FILL, np.uint8) for p, o, m in self._spans(addr, n)]
        return np.concatenate(out)

    def write(self, addr, data):
        k = 0
        for p, o, m in self._spans(addr, len(data)):
            self.pages.setdefault(p, np.full(PAGE, F.FILL, np.uint8))[o:o + m] = data[k:k + m]
            k += m

    def clean(self):
        """the sweep: every byte is FILL"""
        return all((pg == F.FILL).all() for pg in self.pages.values())


def logical(t, seed=0):
    """one block of bytes per far index tuple, never the fill byte"""
    rng = np.random.default_rng(seed)
    return {idx: rng.integers(0, F.FILL, t.block_bytes, dtype=np.uint8) for idx in t.outer_indices()}


def restore(arena, t):
    for idx in t.outer_indices():
        arena.write(F.block_start(t, idx), np.full(t.block_bytes, F.FILL, np.uint8))


def run(op, t, model):
    """-> (values check passed, sweep passed) of access ``op`` on tensor ``t`` under ``model``"""
    arena, data = SparseArena(F.ARENA_BYTES), logical(t)
    want = data
    if op == "read":
        for idx, blk in data.items():  # the test fills its input through torch: exact
            arena.write(F.block_start(t, idx), blk)
        got = {idx: arena.read(F.block_start(t, idx, model), t.block_bytes) for idx in data}
    else:
        if op == "update":
            for idx, blk in data.items():
                arena.write(F.block_start(t, idx), blk)
            want = {idx: blk + 1 for idx, blk in data.items()}
        for idx, blk in data.items():
            if op == "update":
                a = F.block_start(t, idx, model)
                arena.write(a, arena.read(a, t.block_bytes) + 1)
            else:
                if op == "stray":
                    arena.write(F.block_start(t, idx, model), blk)
                    arena.write(F.block_start(t, idx), blk)
                else:
                    arena.write(F.block_start(t, idx, model), blk)
        got = {idx: arena.read(F.block_start(t, idx), t.block_bytes) for idx in data}  # to_numpy copies logical elements
    values = all(np.array_equal(got[idx], want[idx]) for idx in data)
    restore(arena, t)
    return values, arena.clean()


def _tensors():
    """the distinct tensors of the table (many layouts share one), with a layout each belongs to"""
    seen = {}
    for layout in F.TABLE.values():
        for t in layout.t.values():
            seen.setdefault((t.esz, t.base, t.shape, t.strides), (layout.name, t))
    return list(seen.values())


TENSORS = _tensors()
OPS = ("read", "write", "update", "stray")
CAUGHT_BY = {"read": (False, True), "write": (False, False), "update": (False, False), "stray": (True, False)}


@pytest.mark.parametrize("op", OPS)
def test_exact_addressing_passes_both_checks(op):
    for name, t in TENSORS:
        assert run(op, t, "exact") == (True, True), (name, t)


@pytest.mark.parametrize("model", [m for m in F.MODELS if m != "exact"])
@pytest.mark.parametrize("op", OPS)
def test_wrong_addressing_is_rejected_wherever_it_moves_a_block(op, model):
    n = 0
    for name, t in TENSORS:
        if not F.moved(t, model):
            continue
        n += 1
        values, sweep = run(op, t, model)
        assert not (values and sweep), (name, t, "passed both checks")
        assert (values, sweep) == CAUGHT_BY[op], (name, t, values, sweep)  # as the module docstring tabulates
    assert n, "no layout on which this model moves a block"
