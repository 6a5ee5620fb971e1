"""The sizing of dense_prune_kernel's resident workgroups (aoc_dense_split_sizing, aoc_set_dense_share), without a GPU.

1. The library's sizing against the rules include/aoc_hip.h states, restated here from that text: G = budget x share / 256 rounded down to
   a multiple of 8 (from 8 up), at least 1, at most the items; the splits fill whole rounds of G best, over up to three rounds (two at the
   whole share); items = query blocks x splits.
2. The kernel's walk lin = w, w + G, ... and its lin -> (query block, split) map, restated: every item exactly once, and a workgroup of a
   grid that is a multiple of 8 stays inside one XCD's contiguous range of the split-major list.
3. The share setter refuses values outside 1 .. 256 and leaves the value in force alone."""
import ctypes

import pytest

import aoc_amd

OK, INVALID_ARG = 0, -1
M_VALUES = (150, 513, 1100, 25773)
BUDGETS = (0, 1, 2, 3, 7, 9, 64, 224)
SHARES = (256, 224, 192, 160, 128, 37, 1)


def sizing(m, budget, share):
    L = aoc_amd._lib.lib()
    s, i, g = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int32(-1)
    assert L.aoc_dense_split_sizing(m, budget, share, ctypes.byref(s), ctypes.byref(i), ctypes.byref(g)) == OK
    return s.value, i.value, g.value


def floor8(g):
    return g & ~7 if g >= 8 else g


def restated(m, budget, share):
    row_blocks = (m + 511) // 512
    g = max(1, floor8((budget if budget > 0 else 256) * share // 256))
    best, best_eff = 1, 0.0
    for k in range(1, (2 if share == 256 else 3) + 1):
        ns = min(64, max(1, g * k // row_blocks))
        blocks = row_blocks * ns
        eff = blocks / (float(g) * ((blocks + g - 1) // g))
        if eff >= best_eff - 0.005:
            best_eff, best = max(eff, best_eff), ns
    items = row_blocks * best
    return best, items, floor8(min(g, items))


@pytest.mark.parametrize("m", M_VALUES)
def test_sizing_obeys_the_rules(m):
    for budget in BUDGETS:
        for share in SHARES:
            splits, items, g = sizing(m, budget, share)
            what = f"m={m} budget={budget} share={share}: splits={splits} items={items} G={g}"
            assert (splits, items, g) == restated(m, budget, share), what
            assert 1 <= splits <= 64 and items == (m + 511) // 512 * splits, what
            assert 1 <= g <= items and g <= max(1, (budget or 256) * share // 256), what
            assert g < 8 or g % 8 == 0, what


def test_sizing_points():
    """The bench's shape (51 query blocks under a 224-CU mask) and the cases the GPU test relies on."""
    assert sizing(25773, 224, 256) == (8, 408, 224)            # the whole budget: the splits of the one-workgroup-per-item kernel
    assert sizing(25773, 224, 192) == (9, 459, 168)
    assert sizing(25773, 224, 160) == (8, 408, 136)            # three full rounds
    assert sizing(150, 0, 256) == (64, 64, 64)                 # G = items
    assert sizing(1100, 64, 256) == (42, 126, 64)              # G < items, with a remainder
    assert sizing(1100, 1, 256) == (1, 3, 1)                   # one workgroup walks everything
    assert sizing(150, 3, 224) == (6, 6, 2)                    # fewer than 8 items
    for bad in ((0, 0, 256), (150, -1, 256), (150, 0, 0), (150, 0, 257)):
        v = ctypes.c_int32()
        assert aoc_amd._lib.lib().aoc_dense_split_sizing(*bad, ctypes.byref(v), ctypes.byref(v), ctypes.byref(v)) == INVALID_ARG
    assert aoc_amd._lib.lib().aoc_dense_split_sizing(150, 0, 256, None, None, None) == INVALID_ARG


GPU_COMBOS = [(1, 256), (3, 224), (7, 256), (9, 128), (64, 192), (64, 256), (0, 1), (0, 160)]        # (budget, share) of test_gpu_dense_share.py


def test_gpu_combinations_reach_every_kind_of_walk():
    import carried_state_cases as cs
    kinds = {m: set() for m in cs.BUDGET_M}
    for m in cs.BUDGET_M:
        assert sizing(m, 0, 256) == (64, 64 * ((m + 511) // 512), 64 * ((m + 511) // 512))      # the base run: one workgroup per item
        kinds[m].add("grid = items")
        for budget, share in GPU_COMBOS:
            splits, items, g = sizing(m, budget, share)
            if g == 1 and items > 1:
                kinds[m].add("one workgroup walks everything")
            if 1 < g < items and items % g:
                kinds[m].add("remainder")
            if g == items:
                kinds[m].add("grid = items")
            if items < 8:
                kinds[m].add("fewer than 8 items")
            if g >= 8 and items > 2 * g:
                kinds[m].add("three rounds")
    for m, got in kinds.items():
        assert got >= {"one workgroup walks everything", "grid = items", "fewer than 8 items"}, (m, got)
    # (the rule picks splits that fill whole rounds, so a ragged last round needs a query-block count that does not divide them: three blocks)
    assert "remainder" in kinds[1100] and "three rounds" in kinds[1100]


def item_of(lin, nbx, ns):
    """dense_prune_kernel: item lin of the walk -> (query block bx, split by)."""
    nb = nbx * ns
    xcd, slot, q, r = lin & 7, lin >> 3, nb >> 3, nb & 7
    v = (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + slot
    return v % nbx, v // nbx


def test_walk_visits_every_item_once():
    seen_shapes = set()
    for m in M_VALUES:
        for budget in BUDGETS:
            for share in SHARES:
                splits, items, g = sizing(m, budget, share)
                if (m, splits, g) in seen_shapes:
                    continue
                seen_shapes.add((m, splits, g))
                nbx = (m + 511) // 512
                visited = {}
                for w in range(g):
                    ranges = set()
                    for lin in range(w, items, g):
                        bx, by = item_of(lin, nbx, splits)
                        assert 0 <= bx < nbx and 0 <= by < splits
                        assert (bx, by) not in visited, f"m={m} splits={splits} G={g}: item {(bx, by)} twice"
                        visited[(bx, by)] = w
                        ranges.add(lin & 7)
                    assert g < 8 or len(ranges) == 1, "a workgroup of a grid of 8 k leaves its XCD's range"
                assert len(visited) == items, f"m={m} splits={splits} G={g}: {items - len(visited)} items never visited"
    assert len(seen_shapes) > 40


def test_share_setter_rejects_out_of_range_and_recovers():
    L, ops = aoc_amd._lib.lib(), aoc_amd.ops
    before = L.aoc_dense_share()
    assert 1 <= before <= 256
    try:
        assert ops.set_stream_cus(dense_share=192) == 192 == L.aoc_dense_share()
        for bad in (0, -1, 257, 1 << 20):
            assert L.aoc_set_dense_share(bad) == INVALID_ARG
            assert L.aoc_dense_share() == 192, "a refused value changed the share"
            with pytest.raises(aoc_amd._lib.AocHipError):
                ops.set_stream_cus(dense_share=bad)
        assert L.aoc_set_dense_share(1) == OK and L.aoc_dense_share() == 1
        assert L.aoc_set_dense_share(256) == OK and ops.set_stream_cus() == 256
    finally:
        assert L.aoc_set_dense_share(before) == OK
