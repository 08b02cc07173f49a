"""Reference for embedded render vertices (SPEC.md 6b): plain numpy float32, elementwise, in the spec's bracketing. numpy neither
contracts a product and a sum into an FMA nor flushes denormals, so the GPU must reproduce this bit for bit from the same positions."""
import numpy as np


def embedded_ref(x, cage, w):
    """r = ((w0 x[i0] + w1 x[i1]) + w2 x[i2]) + w3 x[i3] per component: every product rounded to binary32, the sums left to right."""
    x = np.ascontiguousarray(x, np.float32).reshape(-1, 3)
    c = np.asarray(cage, np.int64).reshape(-1, 4)
    w = np.ascontiguousarray(w, np.float32).reshape(-1, 4)
    p = [w[:, j:j + 1] * x[c[:, j]] for j in range(4)]
    assert all(q.dtype == np.float32 for q in p)
    return ((p[0] + p[1]) + p[2]) + p[3]


def embedded_ref64(x, cage, w):
    """The same sum in float64 (what embedded_ref is checked against)."""
    x = np.asarray(x, np.float64).reshape(-1, 3)
    c = np.asarray(cage, np.int64).reshape(-1, 4)
    w = np.asarray(w, np.float64).reshape(-1, 4)
    return np.einsum("rj,rjc->rc", w, x[c])


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def lattice_cell_cages(n, cells, rng):
    """Four DISTINCT corners, in random order, of each lattice cell (cx, cy, cz) of jelly_cube(n)."""
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    base = (cells[:, 2] * n + cells[:, 1]) * n + cells[:, 0]
    corner = np.array([dx + dy * n + dz * n * n for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)], np.int64)
    pick = np.argsort(rng.random((cells.shape[0], 8)), axis=1)[:, :4]
    return (base[:, None] + corner[pick]).astype(np.int32)
