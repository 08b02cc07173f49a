"""The bounding box of SPEC.md 6d on the CPU: the two restatements of tests/bounds_ref.py agree on the hostile data, and the box has the
properties the GPU reduction and the group rely on -- it does not depend on the order of the rows, nor on how they are split into chunks
that are reduced on their own and combined. Every comparison is bitwise. (tests/test_abi.py checks that the six entry points are declared,
exported and bound consistently.)"""
import numpy as np
import pytest

from bounds_ref import EMPTY_HI, EMPTY_LO, FLT_MAX, GRID_CAP, SEED, SIZES, SUBNORMAL, bits, bounds_loop, bounds_ref, hostile_rows, is_empty, merge, same_box

LOOP_SIZES = [n for n in SIZES if n <= 1000] + [5000]       # (the sequential twin is a Python loop: the large size is for the GPU)


@pytest.mark.parametrize("nan_z", [False, True])
@pytest.mark.parametrize("n", LOOP_SIZES)
def test_the_two_restatements_agree_on_the_hostile_rows(n, nan_z):
    p = hostile_rows(n, SEED, nan_z=nan_z)
    box = bounds_ref(p)
    assert box[0].dtype == np.float32 and box[1].dtype == np.float32 and box[0].shape == (3,)
    assert same_box(box, bounds_loop(p))
    assert not np.isnan(box[0]).any() and not np.isnan(box[1]).any()
    if nan_z:
        assert is_empty(box, 2) and not is_empty(box, 0) and not is_empty(box, 1)


def test_the_hostile_rows_reach_every_planted_case():
    """Conditions on the inputs: over the sizes the GPU test runs, every planted value is the extreme of some component, the extremes sit in
    a first row, a last row and a row of the last partial wave, and the largest size walks the capped grid three times with a ragged tail
    whose last row holds an extreme."""
    seen, where = set(), set()
    for n in SIZES:
        p = hostile_rows(n, SEED)
        lo, hi = bounds_ref(p)
        for c in range(3):
            col = p[:, c]
            if lo[c] == -FLT_MAX:
                seen.add("-FLT_MAX")
            if hi[c] == FLT_MAX:
                seen.add("+FLT_MAX")
            if hi[c] == -SUBNORMAL:
                seen.add("subnormal")
            if lo[c] == 0 and {0x00000000, 0x80000000} <= set(bits(col[col == 0]).tolist()):
                assert bits(lo)[c] == 0, "a zero result is +0"
                seen.add("signed zeros")
            if lo[c] == -np.inf:
                seen.add("-inf")
            if hi[c] == np.inf:
                seen.add("+inf")
            if np.isnan(col).any():
                seen.add("NaN")
            for r in (int(np.nanargmin(col)), int(np.nanargmax(col))):
                where.add("first" if r == 0 else "last" if r == n - 1 else "last wave" if r >= ((n - 1) // 64) * 64 else "inside")
    assert seen == {"-FLT_MAX", "+FLT_MAX", "subnormal", "signed zeros", "-inf", "+inf", "NaN"}, seen
    assert where == {"first", "last", "last wave", "inside"}, where
    n = SIZES[-1]
    assert n == 3 * GRID_CAP * 256 + 77 and n // (GRID_CAP * 256) == 3 and n % 256 != 0
    p = hostile_rows(n, SEED)
    assert any(int(np.nanargmax(p[:, c])) == n - 1 or int(np.nanargmin(p[:, c])) == n - 1 for c in range(3))


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_the_box_does_not_depend_on_the_order_of_the_rows(seed):
    n = 1000
    p = hostile_rows(n, seed)
    want = bounds_ref(p)
    rng = np.random.default_rng(seed)
    for _ in range(4):
        q = p[rng.permutation(n)]
        assert same_box(bounds_ref(q), want) and same_box(bounds_loop(q), want)
    # -0 met before +0 and the other way round: the comparisons keep whichever came first, the + 0.0f makes both +0
    z = np.abs(hostile_rows(64, seed)) + np.float32(1)
    z[5] = np.float32(-0.0); z[40] = np.float32(0.0)
    a = bounds_loop(z)
    z[[5, 40]] = z[[40, 5]]
    b = bounds_loop(z)
    assert same_box(a, b) and same_box(a, bounds_ref(z)) and not bits(a[0]).any()
    # ... on the maximum as well
    z = -z
    a = bounds_loop(z)
    z[[5, 40]] = z[[40, 5]]
    assert same_box(a, bounds_loop(z)) and same_box(a, bounds_ref(z)) and not bits(a[1]).any()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_box_of_chunks_combines_to_the_box_of_the_whole(seed):
    """What the two kernels (lanes, waves, workgroups, the final pass) and a group (ranks) do: reduce parts, then reduce the results."""
    rng = np.random.default_rng(seed)
    for n in (1, 65, 257, 1000, 70001):
        for nan_z in (False, True):
            p = hostile_rows(n, seed, nan_z=nan_z)
            want = bounds_ref(p)
            for parts in (1, 2, 7, 64, 256):
                cuts = np.sort(rng.integers(0, n + 1, parts - 1))                       # (some chunks are empty)
                chunks = np.split(p, cuts)
                assert same_box(merge([bounds_ref(c) for c in chunks]), want)
            # strided parts, as the lanes of a grid-stride loop see the rows; then the parts' boxes in two levels
            lanes = [bounds_ref(p[k::256]) for k in range(256)]
            waves = [merge(lanes[w:w + 64]) for w in range(0, 256, 64)]
            assert same_box(merge(waves), want)


def test_no_rows_give_the_empty_box():
    for f in (bounds_ref, bounds_loop):
        lo, hi = f(np.zeros((0, 3), np.float32))
        assert np.array_equal(bits(lo), bits(EMPTY_LO)) and np.array_equal(bits(hi), bits(EMPTY_HI))
    lo, hi = merge([bounds_ref(np.zeros((0, 3), np.float32))] * 3)
    assert np.array_equal(bits(lo), bits(EMPTY_LO)) and np.array_equal(bits(hi), bits(EMPTY_HI))
    # a component with NaN only is empty, the others are not
    p = np.float32([[1, np.nan, 3], [-2, np.nan, np.nan]])
    box = bounds_ref(p)
    assert same_box(box, bounds_loop(p)) and is_empty(box, 1) and not is_empty(box, 0) and same_box(box, (np.float32([-2, np.inf, 3]), np.float32([1, -np.inf, 3])))
