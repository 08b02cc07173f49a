"""Reference for the bounding box (SPEC.md 6d) in numpy, and a plain sequential twin of it. Minimum and maximum are exact, a NaN component
never wins a comparison, and the final + 0.0f makes a zero result +0: the box is then a function of the multiset of values alone, so the GPU
must reproduce it bit for bit from the same rows, whatever tree it reduces in."""
import numpy as np

F32 = np.float32
EMPTY_LO = np.full(3, np.inf, F32)
EMPTY_HI = np.full(3, -np.inf, F32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bounds_ref(p):
    """(lo, hi), float32 (3,), of the rows of p (rows, 3): fmin / fmax ignore a NaN operand, the initial value is the empty box."""
    p = np.ascontiguousarray(p, F32).reshape(-1, 3)
    lo = np.array([np.fmin.reduce(p[:, c], initial=np.inf) for c in range(3)], F32)
    hi = np.array([np.fmax.reduce(p[:, c], initial=-np.inf) for c in range(3)], F32)
    return lo + F32(0), hi + F32(0)


def bounds_loop(p):
    """The statements of SPEC.md 6d, one row after the other."""
    p = np.ascontiguousarray(p, F32).reshape(-1, 3)
    lo = [F32(np.inf)] * 3
    hi = [F32(-np.inf)] * 3
    for row in p:
        for c in range(3):
            if row[c] < lo[c]:
                lo[c] = row[c]
            if row[c] > hi[c]:
                hi[c] = row[c]
    return np.array([v + F32(0) for v in lo], F32), np.array([v + F32(0) for v in hi], F32)


def merge(boxes):
    """Boxes of parts -> the box of the whole: min / max again, then + 0.0f (what a group does with its ranks' boxes)."""
    los = np.stack([b[0] for b in boxes]).astype(F32)
    his = np.stack([b[1] for b in boxes]).astype(F32)
    return np.fmin.reduce(los, axis=0, initial=np.inf).astype(F32) + F32(0), np.fmax.reduce(his, axis=0, initial=-np.inf).astype(F32) + F32(0)


def same_box(got, want):
    return np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))


def is_empty(box, c):
    return box[0][c] == np.inf and box[1][c] == -np.inf


FLT_MAX = np.finfo(F32).max
SUBNORMAL = F32(2.0 ** -140)


def hostile_rows(n, seed=0, nan_z=False):
    """(n, 3) float32 in U(-100, 100) with the hostile values planted by a rule seeded with (seed, n). The three components take three
    roles, rotated by the seeded draw:
      A: -FLT_MAX in one row and +FLT_MAX in another
      B: every value positive, the minimum a -0.0 in one row and a +0.0 in another, so lo must come out +0
      C: every value below -1, the maximum a negative subnormal
    plus a row with NaN in y only and a row (+inf, -inf, NaN), whose infinities become extremes of x and y (and hide what the role planted
    there: which role that hits varies with the rotation). The rows are drawn from: the last row, the first row, a row of the last partial
    wave, five random ones; a small n keeps what fits. The reference is computed on the array itself, so every size is a valid case.
    nan_z: the z column is NaN throughout (an empty box in z, finite or infinite ones in x and y)."""
    rng = np.random.default_rng([seed, n])
    p = rng.uniform(-100.0, 100.0, size=(n, 3)).astype(F32)
    a, b, c = (int(v) for v in np.roll([0, 1, 2], int(rng.integers(0, 3))))
    p[:, b] = np.abs(p[:, b]) + F32(1)
    p[:, c] = -np.abs(p[:, c]) - F32(1)
    last_wave = ((n - 1) // 64) * 64
    rows = []
    for r in [n - 1, 0, int(rng.integers(last_wave, n))] + [int(r) for r in rng.integers(0, n, 5)]:
        if r not in rows:
            rows.append(r)
    # the five extremes go, in a drawn order, to the last row, the first row, the row of the last wave and two random rows; the NaN row
    # and the row of infinities to further random rows
    plant = [["a+", "c", "b-0", "b+0", "a-"][i] for i in rng.permutation(5)] + ["nan_y", "inf"]
    for kind, r in zip(plant, rows):
        if kind == "a+":
            p[r, a] = FLT_MAX
        elif kind == "a-":
            p[r, a] = -FLT_MAX
        elif kind == "c":
            p[r, c] = -SUBNORMAL
        elif kind == "b-0":
            p[r, b] = F32(-0.0)
        elif kind == "b+0":
            p[r, b] = F32(0.0)
        elif kind == "nan_y":
            p[r, 1] = np.nan
        else:
            p[r] = (np.inf, -np.inf, np.nan)
    if nan_z:
        p[:, 2] = np.nan
    return p


# the sizes the GPU test runs: around one wave and one workgroup, several workgroups, and three full walks of the capped grid with a ragged tail
SEED = 3                        # the seed of the GPU cases (test_render_bounds.py checks what they reach)
GRID_CAP = 2048                 # = kBoundsMaxGroups of readback_kernels.hip.hpp (workgroups of 256 lanes)
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000, 3 * (GRID_CAP * 256) + 77)
